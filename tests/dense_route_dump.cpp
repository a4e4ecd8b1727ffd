// Stand-alone dump of the dense apply's schedule and of the plan-time form choice (climate_toolbox_amd/csrc/wagg_dense_route.h):
// one line per case, the case's factors before the bar and the decision behind it.  tests/test_dense_route_host.py compares
// the output with tests/golden/dense_routes.json.
//
//   groups   every launch of a batch of T rows, "row0+rows=n_mb x MT": T = 1 .. 4096 and the edges around dense_rows_max
//            line by line, then the FNV-1a of the lines of T = 1 .. 200,000
//   ksplit   a reduced set of (items, n_kt), then the hash of the full product
//   route    dense_launch_route: a reduced set (base cases varied one factor at a time), then the hash of the full product
//   largest  dense_largest_group_route of a few plans
//   form     the form a table takes: the booleans only (the costs are doubles whose last bits depend on the compiler's
//            contraction rules); the program fails if winner and runner-up of a case are closer than a factor 1.05
//
//   dense_route_dump --full   the full products themselves, a line per case
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../climate_toolbox_amd/csrc/wagg_dense_route.h"

using namespace wagg;

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    long long lines = 0;
    void add(const char *s, int n) { for (int i = 0; i < n; ++i) { h ^= (unsigned char)s[i]; h *= 1099511628211ull; } ++lines; }
};

// ---- row groups: what dense_apply launches for T rows -- groups of dense_rows_max rows, each cut by dense_row_groups ----------
static int format_groups(int elem, int64_t Tn, char *buf, size_t n) {
    int at = snprintf(buf, n, "groups e%d T%lld |", elem, (long long)Tn);
    const int64_t rows_max = dense_rows_max(elem);
    for (int64_t t0 = 0; t0 < Tn; t0 += rows_max) {
        const DenseRowGroups gs = dense_row_groups(elem, Tn - t0 < rows_max ? Tn - t0 : rows_max);
        for (int i = 0; i < gs.n && at < (int)n; ++i)
            at += snprintf(buf + at, n - at, " %lld+%lld=%dx%d", (long long)(t0 + gs.g[i].row0), (long long)gs.g[i].rows, gs.g[i].n_mb, gs.g[i].MT);
    }
    if (at < (int)n) at += snprintf(buf + at, n - at, "\n");
    return at;
}

static void groups(bool full) {
    static char buf[4096];
    for (int elem = 4; elem <= 8; elem += 4) {
        const int64_t rm = dense_rows_max(elem);
        if (!full) {
            for (int64_t Tn = 1; Tn <= 4096; ++Tn) { format_groups(elem, Tn, buf, sizeof(buf)); fputs(buf, stdout); }
            const int64_t edges[] = {rm - 1, rm, rm + 1, 2 * rm + 1, 547500};
            for (int64_t Tn : edges) { format_groups(elem, Tn, buf, sizeof(buf)); fputs(buf, stdout); }
        }
        Fnv f;
        for (int64_t Tn = 1; Tn <= 200000; ++Tn) {
            const int n = format_groups(elem, Tn, buf, sizeof(buf));
            f.add(buf, n);
            if (full) fputs(buf, stdout);
        }
        if (!full) printf("groups_full e%d %lld %016llx\n", elem, f.lines, (unsigned long long)f.h);
    }
}

// ---- pick_ksplit -----------------------------------------------------------------------------------------------------------
static void ksplit(bool full) {
    static const int KTS[] = {1, 31, 32, 255, 256, 511, 512, 2047, 2048, 8100};
    static const int ITEMS[] = {1, 2, 3, 4, 5, 8, 12, 16, 24, 31, 32, 33, 48, 63, 64, 95, 96, 97, 128, 192, 256, 384, 512, 1024};
    char buf[128];
    if (!full)
        for (int items : ITEMS) {                      // a line per `items`: S at every n_kt of KTS
            printf("ksplit i%d |", items);
            for (int n_kt : KTS) printf(" kt%d:%d", n_kt, pick_ksplit(items, n_kt));
            printf("\n");
        }
    Fnv f;
    for (int items = 1; items <= 1024; ++items)
        for (int n_kt : KTS) {
            const int n = snprintf(buf, sizeof(buf), "ksplit i%d kt%d | S=%d\n", items, n_kt, pick_ksplit(items, n_kt));
            f.add(buf, n);
            if (full) fputs(buf, stdout);
        }
    if (!full) printf("ksplit_full %lld %016llx\n", f.lines, (unsigned long long)f.h);
}

// ---- dense_launch_route ----------------------------------------------------------------------------------------------------
struct Case {
    int elem = 4, tiled = 0, spmm = 0, maxima = 1, image = 1, exact = 0;
    int gmod = 0;                                // G = n_kt x BK - gmod: 0 = whole k tiles
    int n_mb = 1, mt = 1;                        // mt: index into the MTs at and beside the pack-free threshold
    int aligned = 1, xf = 0, nonfinite = 0, ks = 0;
};
static const int MTS32[4] = {4, 18, 20, 21}, MTS64[4] = {4, 8, 10, 11};
static const int XF[3] = {0, 3, -1};             // plain, a power, degree days
static const int KS[3] = {0, 8, 24};
constexpr int N_NT = 3, N_KT = 2100;              // (64 k-slices of 32 tiles fit: pick_ksplit has its whole range)

static DensePlanScalars plan_of(const Case &k) {
    DensePlanScalars p;
    p.elem = k.elem; p.n_nt = N_NT; p.n_kt = N_KT; p.G = (int64_t)N_KT * dense_bk(k.elem) - k.gmod;
    p.tiled = k.tiled != 0; p.spmm = k.spmm != 0;
    p.has_maxima = k.maxima != 0; p.has_image = k.image != 0;
    return p;
}
static int format_route(const char *tag, const DenseRoute &r, char *buf, size_t n) {
    static const char *FORM[4] = {"none", "split", "full", "tiled"}, *PF[3] = {"none", "tiled", "full"};
    return snprintf(buf, n, "%s | form=%s S=%d kps=%d img=%d pf=%s nblk=%lld xslots=%lld slab=%zu slabs=%zu xp=%zu xmax=%zu\n", tag, FORM[r.form & 3],
                    r.S, r.kt_per_slice, (int)r.image, PF[r.pack_free % 3], (long long)r.nblk, (long long)r.x_slots, r.slab_words, r.slabs_words,
                    r.xp_words, r.xmax_words);
}
static int format_case(const Case &k, char *buf, size_t n) {
    const DensePlanScalars p = plan_of(k);
    DenseCall c;
    c.MT = (k.elem == 8 ? MTS64 : MTS32)[k.mt]; c.n_mb = k.n_mb; c.rows = (int64_t)c.n_mb * c.MT * 16 - 5;
    c.ksplit = KS[k.ks]; c.exact = k.exact != 0; c.xf_mode = XF[k.xf]; c.aligned16 = k.aligned != 0; c.nonfinite_met = k.nonfinite != 0;
    char tag[160];
    snprintf(tag, sizeof(tag), "route e%d tl%d sp%d mx%d im%d ex%d g%d mb%d mt%d a%d xf%d nf%d ks%d", k.elem, k.tiled, k.spmm, k.maxima, k.image,
             k.exact, k.gmod, k.n_mb, c.MT, k.aligned, c.xf_mode, k.nonfinite, c.ksplit);
    return format_route(tag, dense_launch_route(p, c), buf, n);
}

static void routes(bool full) {
    char buf[512];
    static const int MBS[3] = {1, 2, 4};
    if (!full) {
        auto emit = [&](const Case &k) { format_case(k, buf, sizeof(buf)); fputs(buf, stdout); };
        // base cases: split (fp32 with maxima), exact full form in both types, tile-sparse in both types -- each at one and at
        // four row blocks of the threshold MT -- then one factor at a time
        for (int elem = 4; elem <= 8; elem += 4)
            for (int kind = 0; kind < 3; ++kind)
                for (int mb = 0; mb < 3; mb += 2) {
                    Case b;
                    b.elem = elem; b.n_mb = MBS[mb]; b.mt = 2;
                    if (kind == 1) b.exact = 1;
                    if (kind == 2) { b.tiled = 1; b.maxima = 0; b.image = 0; }
                    if (elem == 8) { b.maxima = 0; b.image = 0; }
                    if (elem == 8 && kind == 0) continue;                   // (fp64 has no split form: its default is kind 1's route)
                    emit(b);
                    Case v;
                    v = b; v.n_mb = 2; emit(v);
                    for (int m = 0; m < 4; ++m) if (m != b.mt) { v = b; v.mt = m; emit(v); }
                    v = b; v.aligned = 0; emit(v);
                    for (int x = 1; x < 3; ++x) { v = b; v.xf = x; emit(v); }
                    v = b; v.nonfinite = 1; emit(v);
                    v = b; v.gmod = 1; emit(v);
                    for (int s = 1; s < 3; ++s) { v = b; v.ks = s; emit(v); }
                    v = b; v.image = !b.image; emit(v);
                    v = b; v.maxima = !b.maxima; emit(v);
                    v = b; v.spmm = 1; emit(v);
                }
    }
    Fnv f;
    Case k;
    for (k.elem = 4; k.elem <= 8; k.elem += 4)
    for (k.tiled = 0; k.tiled < 2; ++k.tiled)
    for (k.spmm = 0; k.spmm < 2; ++k.spmm)
    for (k.maxima = 0; k.maxima < 2; ++k.maxima)
    for (k.image = 0; k.image < 2; ++k.image)
    for (k.exact = 0; k.exact < 2; ++k.exact)
    for (k.gmod = 0; k.gmod < 2; ++k.gmod)
    for (int mb = 0; mb < 3; ++mb)
    for (k.mt = 0; k.mt < 4; ++k.mt)
    for (k.aligned = 0; k.aligned < 2; ++k.aligned)
    for (k.xf = 0; k.xf < 3; ++k.xf)
    for (k.nonfinite = 0; k.nonfinite < 2; ++k.nonfinite)
    for (k.ks = 0; k.ks < 3; ++k.ks) {
        k.n_mb = MBS[mb];
        const int n = format_case(k, buf, sizeof(buf));
        f.add(buf, n);
        if (full) fputs(buf, stdout);
    }
    if (!full) printf("route_full %lld %016llx\n", f.lines, (unsigned long long)f.h);
    if (full) return;
    // the launch group a plan's W image is sized against
    for (int i = 0; i < 4; ++i) {
        Case k2;
        k2.elem = i == 3 ? 8 : 4; k2.tiled = i == 1; k2.spmm = i == 2; k2.maxima = i == 0; k2.image = 0;
        char tag[64];
        snprintf(tag, sizeof(tag), "largest e%d tl%d sp%d mx%d", k2.elem, k2.tiled, k2.spmm, k2.maxima);
        format_route(tag, dense_largest_group_route(plan_of(k2)), buf, sizeof(buf));
        fputs(buf, stdout);
    }
}

// ---- the form of a caller's table ------------------------------------------------------------------------------------------
// Tables on the c5 grid (G = 1,036,800 cells, R = 24,378 regions: 96 column tiles, 36 region blocks of the entry-list form
// with 8,100 chunks of 16 lists each): `stored` per mille of the tiles hold a pair, `walked` million entries are walked.
// Well inside each form, and either side of each of the three crossovers.
struct FormCase { const char *name; int elem, n_nt, n_rb, stored_pm; int64_t walked_m; };
static const FormCase FORMS[] = {
    {"full-inside", 4, 96, 36, 1000, 20000},       {"tiled-inside", 4, 96, 36, 30, 20000},       {"entries-inside", 4, 96, 36, 1000, 100},
    {"full|tiled:full", 4, 96, 36, 450, 20000},    {"full|tiled:tiled", 4, 96, 36, 250, 20000},
    {"full|entries:full", 4, 96, 36, 1000, 2800},  {"full|entries:entries", 4, 96, 36, 1000, 700},
    {"tiled|entries:tiled", 4, 96, 36, 100, 1100}, {"tiled|entries:entries", 4, 96, 36, 100, 250},
    // three column tiles fill 192 of 256 CUs in the full form: the same share of stored tiles then goes the other way
    {"wide-400:full", 4, 96, 36, 400, 20000},      {"narrow-400:tiled", 4, 3, 1, 400, 20000},
    // (fp64: the tile-sparse kernel is the faster of the two MFMA forms at any share of stored tiles)
    {"f64-tiled-inside", 8, 96, 36, 30, 40000},    {"f64-entries-inside", 8, 96, 36, 1000, 100},
    {"f64-tiled|entries:tiled", 8, 96, 36, 100, 1600}, {"f64-tiled|entries:entries", 8, 96, 36, 100, 400},
};

static int forms() {
    int bad = 0;
    for (const FormCase &k : FORMS) {
        const int64_t G = 1036800;
        const int n_nt = k.n_nt, n_rb = k.n_rb;
        const int64_t n_kt = G / dense_bk(k.elem), n_all = n_kt * n_nt, n_lists = (int64_t)n_rb * 8100 * 16;
        const FormCost c = table_form_cost(G, k.elem, n_all * k.stored_pm / 1000, n_all, k.walked_m * 1000000, n_rb, n_lists, n_nt);
        bool tiled = false, entries = false;
        pick_table_form(c, &tiled, &entries);
        double t[3] = {c.t_full, c.t_tiled, c.t_entries};
        for (int i = 0; i < 3; ++i)
            for (int j = i + 1; j < 3; ++j)
                if (t[j] < t[i]) { const double s = t[i]; t[i] = t[j]; t[j] = s; }
        if (!(t[1] >= 1.05 * t[0])) {
            fprintf(stderr, "form case %s: winner and runner-up within 5 %% (%.4g %.4g %.4g)\n", k.name, c.t_full, c.t_tiled, c.t_entries);
            bad = 1;
        }
        printf("form %s e%d nt%d stored%d walked%lld | tiled=%d entries=%d\n", k.name, k.elem, k.n_nt, k.stored_pm, (long long)k.walked_m, (int)tiled, (int)entries);
    }
    return bad;
}

int main(int argc, char **argv) {
    const bool full = argc > 1 && !strcmp(argv[1], "--full");
    groups(full);
    ksplit(full);
    routes(full);
    return full ? 0 : forms();
}
