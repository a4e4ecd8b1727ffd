// Stand-alone dump of the segment-table route (climate_toolbox_amd/csrc/wagg_route.h): one line per case, the case's
// factors before the bar and every field of its SparseRoute behind it.  tests/test_routes_host.py compares the output with
// tests/golden/routes.json.
//
//   route_dump          the reduced set (every row and bracket of the kernel table as a base case, each varied one factor at a
//                       time), then "full <cases> <FNV-1a of the lines of the full product>"
//   route_dump --full   the full product itself, a line per case
//
// The plans are synthetic: every chunking carries its own n_part (100 + its index) so that ws_rows names the chunking whose
// scalars were read, and the chunkings a plan "does not have" are filled like the others -- a route that reads one shows.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../climate_toolbox_amd/csrc/wagg_route.h"

using namespace wagg;

struct Case {
    int elem = 4, flags = 0, has = 7;            // has: bit 0 has_lines, 1 has_lines64, 2 has_lines64e
    int layout = WAGG_LAYOUT_TG, out_layout = WAGG_OUT_TR;
    int xf = 0;                                  // index into XFS
    int compact = COMPACT_NONE, aligned = 1, gmod = 0;
    int shape = 1;                               // groups: 0 none, 1 all normal, 2 giant + normal, 3 all giant
    int n_empty = 0, cq = 1;                     // cq: the whole-line chunkings carry compact rows (Gc = 48, Gq = 24)
    int64_t Ttot = 65, ldx = -1;                 // ldx < 0: the grid row
};

static const int FLAGS[8] = {0, WAGG_PLAN_NO_LC, WAGG_PLAN_NO_STREAM, WAGG_PLAN_NO_LC | WAGG_PLAN_NO_STREAM, WAGG_PLAN_LC_MFMA,
                             WAGG_PLAN_LC_MFMA | WAGG_PLAN_NO_LC, WAGG_PLAN_LC_MFMA | WAGG_PLAN_NO_STREAM,
                             WAGG_PLAN_LC_MFMA | WAGG_PLAN_NO_LC | WAGG_PLAN_NO_STREAM};
static const struct { const char *name; RouteTransform xf; } XFS[8] = {
    {"none", {RX_NONE, 0, 1}}, {"p1", {RX_POWERS, 1, 1}}, {"p3", {RX_POWERS, 3, 1}}, {"p1x2", {RX_POWERS, 1, 2}},
    {"p1x4", {RX_POWERS, 1, 4}}, {"p1x5", {RX_POWERS, 1, 5}}, {"edd1", {RX_EDD, 0, 1}}, {"edd4", {RX_EDD, 0, 4}}};
static const int SHAPES[4][2] = {{0, 0}, {5, 0}, {5, 2}, {3, 3}};       // n_groups, g0_normal

static int format(const Case &k, char *buf, size_t n) {
    RoutePlan p;
    p.flags = k.flags;
    p.has_lines = k.has & 1; p.has_lines64 = (k.has & 2) != 0; p.has_lines64e = (k.has & 4) != 0;
    p.G = k.gmod ? 62 : 64; p.R = 9;
    for (int ch = 0; ch < 4; ++ch) {
        RouteChunking &d = p.ch[ch];
        d.n_groups = SHAPES[k.shape][0]; d.g0_normal = SHAPES[k.shape][1];
        d.n_part = ch == CH_R ? 0 : 100 + ch;
        d.n_empty = k.n_empty;
        d.Gc = ch != CH_R && k.cq ? 48 : 0; d.Gq = ch != CH_R && k.cq ? 24 : 0;
    }
    RouteCall c;
    c.elem = k.elem; c.layout = k.layout; c.out_layout = k.out_layout; c.xf = XFS[k.xf].xf; c.compact = k.compact;
    c.ldx = k.ldx < 0 ? p.G : k.ldx; c.aligned16 = k.aligned != 0 && (c.ldx * k.elem) % 16 == 0; c.Ttot = k.Ttot;
    const SparseRoute r = sparse_route(p, c);
    static const char *CH[4] = {"R", "L32", "L64", "L64e"}, *MAIN[4] = {"none", "lcv", "lc_mfma", "stream"};
    static const char *FIN[8] = {"none", "fill", "transpose", "transpose+fill", "combine", "?", "?", "?"};
    return snprintf(buf, n, "e%d f%d h%d %s %s %s c%d a%d g%d s%d ne%d cq%d T%lld ldx%lld | ch=%s main=%s vec=%d edd=%d gt=%d planes=%d "
                    "per_power=%d gather=%d gvec=%d gnthr=%d nplanes=%d via_ws=%d ws_rows=%lld fin=%s refuse=%d\n",
                    k.elem, k.flags, k.has, k.layout == WAGG_LAYOUT_TG ? "TG" : "GT", k.out_layout == WAGG_OUT_TR ? "TR" : "RT", XFS[k.xf].name,
                    k.compact, k.aligned, k.gmod, k.shape, k.n_empty, k.cq, (long long)k.Ttot, (long long)c.ldx, CH[r.chunking & 3], MAIN[r.main & 3],
                    (int)r.vec, (int)r.edd, (int)r.gt, r.planes, (int)r.per_power, r.gather_groups, (int)r.gather_vec, r.gather_nthr, r.nplanes,
                    (int)r.via_ws, (long long)r.ws_rows, FIN[r.finish & 7], r.refuse);
}

static void reduced() {
    char buf[512];
    auto emit = [&](const Case &k) { format(k, buf, sizeof(buf)); fputs(buf, stdout); };
    static const int BASE_XF[3] = {0, 4, 7};                            // the rows of the table: none, four powers, four thresholds
    for (int elem = 4; elem <= 8; elem += 4)
        for (int layout = 0; layout < 2; ++layout)
            for (int bx = 0; bx < 3; ++bx) {
                Case b;
                b.elem = elem; b.layout = layout ? WAGG_LAYOUT_GT : WAGG_LAYOUT_TG; b.xf = BASE_XF[bx];
                emit(b);
                Case v;
                for (int i = 1; i < 8; ++i) { v = b; v.flags = FLAGS[i]; emit(v); }
                for (int h = 0; h < 7; ++h) { v = b; v.has = h; emit(v); }
                v = b; v.out_layout = WAGG_OUT_RT; emit(v);
                for (int x = 0; x < 8; ++x) if (x != b.xf) { v = b; v.xf = x; emit(v); }
                for (int cm = 1; cm <= 2; ++cm) {
                    v = b; v.compact = cm; emit(v);
                    v.ldx = 30; emit(v);                                // between Gq and Gc
                    v.ldx = -1; v.cq = 0; emit(v);
                    v.cq = 1; v.shape = 2; emit(v);                     // a giant group: the main kernel leaves it
                }
                v = b; v.aligned = 0; emit(v);
                v = b; v.gmod = 2; emit(v);
                for (int s = 0; s < 4; ++s) if (s != b.shape) { v = b; v.shape = s; emit(v); }
                v = b; v.n_empty = 2; emit(v);
                v.out_layout = WAGG_OUT_RT; emit(v);
                v = b; v.cq = 0; emit(v);
                v = b; v.Ttot = 0; emit(v);
                // the brackets' other side: no whole-line chunking at all, and with each flag on top of that
                // (G % 4 == 2: whole-quad loads of fp64 rows take the clamped arm)
                for (int i = 0; i < 4; ++i) {
                    v = b; v.has = 0; v.flags = FLAGS[i]; v.shape = 2; v.n_empty = 2; emit(v);
                    if (i < 2) { v.gmod = 2; emit(v); }
                }
            }
}

static void full(bool print) {
    char buf[512];
    uint64_t h = 1469598103934665603ull;
    long long cases = 0;
    Case k;
    for (k.elem = 4; k.elem <= 8; k.elem += 4)
    for (int fi = 0; fi < 8; ++fi)
    for (k.has = 0; k.has < 8; ++k.has)
    for (int layout = 0; layout < 2; ++layout)
    for (int ol = 0; ol < 2; ++ol)
    for (k.xf = 0; k.xf < 8; ++k.xf)
    for (k.compact = 0; k.compact < 3; ++k.compact)
    for (k.aligned = 0; k.aligned < 2; ++k.aligned)
    for (k.gmod = 0; k.gmod <= 2; k.gmod += 2)
    for (k.shape = 0; k.shape < 4; ++k.shape)
    for (k.n_empty = 0; k.n_empty <= 2; k.n_empty += 2)
    for (k.cq = 0; k.cq < 2; ++k.cq)
    for (int tt = 0; tt < 2; ++tt) {
        k.flags = FLAGS[fi];
        k.layout = layout ? WAGG_LAYOUT_GT : WAGG_LAYOUT_TG; k.out_layout = ol ? WAGG_OUT_RT : WAGG_OUT_TR;
        k.Ttot = tt ? 65 : 0;
        const int n = format(k, buf, sizeof(buf));
        for (int i = 0; i < n; ++i) { h ^= (unsigned char)buf[i]; h *= 1099511628211ull; }
        if (print) fputs(buf, stdout);
        ++cases;
    }
    if (!print) printf("full %lld %016llx\n", cases, (unsigned long long)h);
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--full")) { full(true); return 0; }
    reduced();
    full(false);
    return 0;
}
