"""Layouts whose rows lie gigabytes apart: the shapes of tests/test_gpu_large_pitch.py, and what a truncated row offset would
read from them.  A plain module (no tests); tests/test_large_pitch_host.py checks it without a GPU.

A (T, G) view sits inside ONE 1-D buffer filled with a finite sentinel: `lead` elements of sentinel, then row r at
``lead + r * pitch``.  Two tiers say what the row offsets outgrow:

  "bytes"   LIMIT = 2^32 bytes (2^32 / elem_bytes elements): a 32-bit BYTE offset wraps;
  "elems"   LIMIT = 2^31 elements: a 32-bit signed ELEMENT index wraps.

``pitch = ceil(LIMIT / (T - 2))`` rounded up to 64 elements, so the rows T - 2 and T - 1 start at or beyond LIMIT and the
rows before them pass LIMIT / 2, where a sign-extended offset turns negative.  64 elements keep rows 16-byte aligned and a
whole number of k tiles (32 cells of fp32, 16 of fp64) apart; ``aligned=False`` adds one element and breaks both.

The lead is what makes a wrong address a wrong NUMBER instead of a fault: an offset cut to 32 bits and sign-extended is
at worst 2^31 (bytes or elements) BELOW the view's base, so the lead holds that many -- LIMIT / 2 elements in the "bytes"
tier, LIMIT elements in the "elems" tier (with LIMIT / 2 there, a sign-extended element index of the rows at and beyond
2^31 would land up to 2^30 elements in front of the allocation; the same holds for any layout whose last row starts 2^31
elements or more from the base).  Every such read then hits sentinel or another row."""
import numpy as np

GIB = 1 << 30
MAX_BYTES = 40 * GIB                    # no buffer of a case is larger
X_SENTINEL = -1e30                      # finite: neither skipped like NaN (S6) nor flagged like +-inf
TRUNCATIONS = ("bytes-zext", "bytes-sext", "elems-zext", "elems-sext")


def limit(elem_bytes, tier):
    if tier == "bytes":
        return (1 << 32) // elem_bytes
    if tier == "elems":
        return 1 << 31
    raise ValueError("tier must be 'bytes' or 'elems'")


def layout(T, G, elem_bytes, tier, aligned=True, planes=1):
    """(lead, pitch, total_elems) of a (T, G) view of `elem_bytes`-byte elements; see the module's docstring.  `planes` > 1:
    a stack of such views `T * pitch` elements apart (the pitch is that of ONE view of T rows) -- planes * T rows in all."""
    if T < 4:
        raise ValueError("T >= 4: two rows at or beyond LIMIT and one between LIMIT / 2 and LIMIT")
    lim = limit(elem_bytes, tier)
    pitch = -(-lim // (T - 2))
    pitch = -(-pitch // 64) * 64 + (0 if aligned else 1)
    if pitch < G:
        raise ValueError("rows of %d elements do not fit a pitch of %d" % (G, pitch))
    lead = lim // 2 if tier == "bytes" else lim
    if (planes * T - 1) * pitch >= 1 << 31:            # (a stack of planes in the "bytes" tier can reach 2^31 elements too)
        lead = max(lead, 1 << 31)
    assert lead % 4 == 0
    return lead, pitch, lead + (planes * T - 1) * pitch + G


def view(torch, big, T, G, lead, pitch):
    return torch.as_strided(big, (T, G), (pitch, 1), storage_offset=lead)


def _s32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >> 31 else v


def wrapped_offsets(off, elem_bytes):
    """{truncation: element offset} for the truncations of TRUNCATIONS that change the element offset `off` (of a row from
    the view's base): the byte offset or the element index cut to 32 bits, zero- or sign-extended"""
    cand = {"bytes-zext": ((off * elem_bytes) & 0xffffffff) // elem_bytes, "bytes-sext": _s32(off * elem_bytes) // elem_bytes,
            "elems-zext": off & 0xffffffff, "elems-sext": _s32(off)}
    return {k: v for k, v in cand.items() if v != off}


def wrapped_positions(T, G, lead, pitch, elem_bytes):
    """For every row r the buffer positions {truncation: position} at which each truncation that alters the row's offset
    r * pitch would start reading it (a row whose offset survives a truncation has no entry for it)"""
    return [{k: lead + v for k, v in wrapped_offsets(r * pitch, elem_bytes).items()} for r in range(T)]


def as_read_through(small, lead, pitch, elem_bytes, truncation, sentinel=X_SENTINEL):
    """The (T, G) field a kernel would see whose row offsets went through `truncation`: rebuilt on the host from the case's
    small data and the sentinel, without the buffer.  Rows the truncation leaves alone are the data's own."""
    small = np.asarray(small)
    T, G = small.shape
    out = np.array(small)
    for r, pos in enumerate(wrapped_positions(T, G, lead, pitch, elem_bytes)):
        if truncation not in pos:
            continue
        p = pos[truncation] + np.arange(G, dtype=np.int64)
        row, col = np.divmod(p - lead, pitch)
        inside = (p >= lead) & (row < T) & (col < G)
        out[r] = np.where(inside, small[np.clip(row, 0, T - 1), np.clip(col, 0, G - 1)], small.dtype.type(sentinel))
    return out
