"""The rule of the paged cache without fp16 pools (include/sageattn_hip_paged_rows.h) restated for the tests in plain Python /
torch: the lengths of a call, the ring of two tile slots as a model on row ids, which bytes a call may write, and the
comparison of a ``SagePagedRowCache`` with the reference -- ``SagePagedKVCache`` over fp16 pools into which the same rows
were written, with the same table."""
import numpy as np
import torch

import kvcache_util as KU
import paged_util as PU

CAP = 512  # the capacity of the walks and of the GPU tests


# ---- lengths ---------------------------------------------------------------------------------------------------------------
def call_geometry(start, length, N=CAP):
    """-> None for a call that touches nothing (len_b == 0), else (s, len, n, keep, t0, tl): keep = min(s, len) rows are the
    cache's own, the touched tiles are t0 .. tl"""
    s, ln = KU.clamp_len(start, N), KU.clamp_len(length, N)
    if ln == 0:
        return None
    return s, ln, max(ln - s, 0), min(s, ln), min(s, ln - 1) >> 6, (ln - 1) >> 6


def ring_home(r):
    """(slot, row) of logical row r in k_tail [B, Hk, 2, 64, D]"""
    return (r >> 6) & 1, r & 63


def ring_written_rows(start, length, N=CAP):
    """the logical rows whose input row the ring must hold after the call: [s, len) within the tiles tl - 1 and tl"""
    g = call_geometry(start, length, N)
    if g is None:
        return range(0)
    s, ln, _, _, _, tl = g
    return range(max(s, 64 * (tl - 1)), ln)


def ring_read_rows(start, length, N=CAP):
    """the logical rows a call takes from the ring: [64 t0, min(s, len))"""
    g = call_geometry(start, length, N)
    if g is None:
        return range(0)
    _, _, _, keep, t0, _ = g
    return range(64 * t0, keep)


# ---- the ring on row ids ---------------------------------------------------------------------------------------------------
class RingModel:
    """One sequence.  ``rows`` is the truth: the id of every logical row; ``ring`` the 128 ring rows; ``hi`` the largest tile
    index any call wrote rows of.  Every row a call writes gets a fresh id, so a stale row of the same index shows."""

    def __init__(self):
        self.rows, self.ring, self.hi, self._next = [], [None] * 128, -1, 0

    def admitted(self, start, length, N=CAP):
        """the precondition: the rows below min(s, len) exist, and t0 >= hi - 1"""
        g = call_geometry(start, length, N)
        if g is None:
            return True
        _, _, _, keep, t0, _ = g
        return keep <= len(self.rows) and t0 >= self.hi - 1

    def append(self, start, length, N=CAP):
        """the call as the kernel makes it -> [(row, id expected, id found)] of the ring reads that found another row"""
        g = call_geometry(start, length, N)
        if g is None:                                                    # no keys left: nothing is read or written
            self.rows = []
            return []
        s, ln, n, keep, _, tl = g
        wrong = []
        for r in ring_read_rows(start, length, N):                       # K slot 0 reads ...
            slot, row = ring_home(r)
            found, want = self.ring[64 * slot + row], self.rows[r] if r < len(self.rows) else ("missing", r)
            if found != want:
                wrong.append((r, want, found))
        self.rows = self.rows[:keep] + [self._next + i for i in range(n)]
        self._next += n
        for r in ring_written_rows(start, length, N):                    # ... and only then writes
            slot, row = ring_home(r)
            self.ring[64 * slot + row] = self.rows[r]
        if n:
            self.hi = max(self.hi, tl)
        return wrong


def first_call_grid(old, N=CAP):
    """Every (s, len) in [0, N]^2 after one call from 0 to ``old`` rows, as arrays [N + 1, N + 1]: (admitted, served) --
    served: every ring row the call reads is the row the first call left there.  Vectorised: the ring after the first call
    holds row r at r & 127 for the rows < old of the tiles tl - 1 and tl."""
    ring = np.full(128, -1)
    for r in ring_written_rows(0, old, N):
        ring[r & 127] = r
    rows = np.arange(N + 1)
    good = np.concatenate([[0], np.cumsum(ring[rows[:N] & 127] == rows[:N])])     # good rows below r
    s, ln = np.meshgrid(rows, rows, indexing="ij")
    keep, t0 = np.minimum(s, ln), np.minimum(s, np.maximum(ln - 1, 0)) >> 6
    hi = (old - 1) >> 6 if old else -1
    admitted = (ln == 0) | ((keep <= old) & (t0 >= hi - 1))
    lo = np.minimum(64 * t0, keep)
    served = (ln == 0) | (good[keep] - good[lo] == keep - lo)
    return admitted, served


# ---- which bytes a call may write ------------------------------------------------------------------------------------------
def token_of_pos(pos):
    """the token inside its 64-token block that byte ``pos`` of a V^T image row holds (the order the P.V MFMA reads)"""
    h, j = pos >> 5, pos & 31
    return 32 * (j >> 4) + (j & 3) + 8 * ((j & 15) >> 2) + 4 * h


def write_masks(cache, table, starts, lens):
    """bool masks on the CPU, True where ONE call may write: (k8, k_scale, v, k_tail) -- k8 and v shaped as the HND views of
    the pools (v: the V^T images for FP8 P.V, else v_pool), k_tail as it is.  K: the rows < len_b and the scales of the touched
    tiles.  V, FP8: the tokens >= min(s_b, len_b) of the blocks t0 .. tl; FP16: the rows [s_b, len_b).  Ring: the rows of
    ``ring_written_rows``."""
    layout, ps, g = cache.tensor_layout, cache.page_size, KU.gpb(cache)
    N = table.shape[1] * ps
    fp8 = cache.pv == "fp8"
    mk = torch.zeros(PU.hnd_pool(cache.k8, layout).shape, dtype=torch.bool)
    ms = torch.zeros(cache.k_scale.shape, dtype=torch.bool)
    mv = torch.zeros(PU.hnd_pool(cache.v, layout).shape, dtype=torch.bool)
    mt = torch.zeros(cache.k_tail.shape, dtype=torch.bool)
    tok = torch.tensor([token_of_pos(p) for p in range(64)])
    for b, (s0, n0) in enumerate(zip(starts, lens)):
        geo = call_geometry(s0, n0, N)
        if geo is None:
            continue
        s, ln, _, keep, t0, tl = geo
        row = table[b].tolist()
        for t in range(t0, tl + 1):
            page, ti = PU.tile_home(row, t, ps)
            mk[page, :, 64 * ti:64 * ti + min(64, ln - 64 * t)] = True
            ms[page, :, g * ti:g * ti + g] = True
            if fp8:
                mv[page, :, :, 64 * ti:64 * ti + 64] |= (64 * t + tok >= keep)
        if not fp8:
            for r in range(s, ln):
                page, ti = PU.tile_home(row, r >> 6, ps)
                mv[page, :, 64 * ti + (r & 63)] = True
        for r in ring_written_rows(s0, n0, N):
            slot, rr = ring_home(r)
            mt[b, :, slot, rr] = True
    return mk, ms, mv, mt


def state_bytes(cache):
    """(k8, k_scale, v, k_tail) as uint8 on the CPU, in the shapes of ``write_masks`` with the element's bytes last"""
    layout = cache.tensor_layout
    as_bytes = lambda t: t.contiguous().view(torch.uint8).view(*t.shape, t.element_size()).cpu()  # noqa: E731
    return (as_bytes(PU.hnd_pool(cache.k8, layout)), as_bytes(cache.k_scale), as_bytes(PU.hnd_pool(cache.v, layout)),
            as_bytes(cache.k_tail))


# ---- the reference's pools -------------------------------------------------------------------------------------------------
def scatter_rows(pool, table, layout, starts, lens, new):
    """what the caller of ``SagePagedKVCache`` does before its append: rows [s_b, len_b) of sequence b <- new[b, :, :n_b]
    (``new`` HND [B, H, T, D]; ``pool`` in ``layout``)"""
    hp = PU.hnd_pool(pool, layout)
    ps = hp.size(2)
    N = table.shape[1] * ps
    for b, (s0, n0) in enumerate(zip(starts, lens)):
        geo = call_geometry(s0, n0, N)
        if geo is None or geo[2] == 0:
            continue
        s, ln = geo[0], geo[1]
        r = torch.arange(s, ln)
        pages = table[b, r // ps].long().to(pool.device)
        hp[pages, :, (r % ps).to(pool.device)] = new[b, :, :ln - s].transpose(0, 1)


def assert_state_equals_ref(cache, ref, table, lens):
    """the statistics, every valid K tile (INT8 rows < len_b, scales), and V: the blocks of the V^T image of every valid tile,
    or the rows < len_b of ``v_pool`` -- bit for bit against the paged reference, page by page (one table)"""
    same = lambda a, b: torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))  # noqa: E731
    assert same(cache.km, ref.km), "km"
    layout, ps, g, fp8 = cache.tensor_layout, cache.page_size, KU.gpb(cache), cache.pv == "fp8"
    if fp8:
        assert same(cache.v_scale, ref.v_scale) and same(cache.v_coef, ref.v_coef), "V statistics"
    k8, rk8 = PU.hnd_pool(cache.k8, layout), PU.hnd_pool(ref.k8, layout)
    v, rv = PU.hnd_pool(cache.v, layout), PU.hnd_pool(ref.v8 if fp8 else ref.v, layout)
    for b, n in enumerate(lens):
        for t in range((n + 63) // 64):
            page, ti = PU.tile_home(table[b].tolist(), t, ps)
            rows = slice(64 * ti, 64 * ti + min(64, n - 64 * t))
            assert same(k8[page, :, rows], rk8[page, :, rows]), ("k8", b, t)
            assert same(cache.k_scale[page, :, g * ti:g * ti + g], ref.k_scale[page, :, g * ti:g * ti + g]), ("k_scale", b, t)
            if fp8:
                assert same(v[page, :, :, 64 * ti:64 * ti + 64], rv[page, :, :, 64 * ti:64 * ti + 64]), ("v8", b, t)
            else:
                assert same(v[page, :, rows], rv[page, :, rows]), ("v_pool", b, t)
