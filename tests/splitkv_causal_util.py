"""The rule of causal split-KV attention (include/sageattn_hip.h, causal split-KV attention) restated in torch for the tests,
and its oracle on the constructed operands of tests/constructed_cases.py.  CPU only; nothing of the library.

The rule.  len_b = clamp(kv_lens[b], 0, N); g = q_fold; T = M / g tokens; row r is token t = r // g; off_b = len_b - T (it may
be negative).  Row r attends the keys 0 <= j <= t + off_b.  Split s owns the tiles [s * tps_b, min((s + 1) * tps_b, ntk_b)),
tps_b = ceil(ntk_b / S), ntk_b = ceil(len_b / 64).  For q-block qb, end_qb = min(len_b, min(128 qb + 127, M - 1) // g + off_b
+ 1) is the key bound of its last row; workgroup (b, h, qb, s) runs iff 64 * s * tps_b < end_qb, and the merge reads
min(count_b, ceil(ceil(end_qb / 64) / tps_b)) slots for every row of the q-block.

The oracle.  A constructed case cut to len_b keys and given the band above as a bool mask (``with_mask``) is again a
constructed case: ``reference64`` is the fp64 softmax of exactly the keys a row attends, and ``bound`` its derived tolerance.
Per split, the same case restricted to the split's tiles with the band's columns of those tiles; the merged tolerance is the
formula of ``constructed_cases.merged_bound`` with one change the rule asks for: a split in which a row keeps no key takes no
part in that row's sums (the merge drops its slot by select).  No new constant."""
import math

import torch

import constructed_cases as C
from splitkv_util import clamp_len, split_range  # noqa: F401  (the ranges are those of the non-causal form)

NEG_INF = float("-inf")


# ---- the rule's bookkeeping --------------------------------------------------------------------------------------------------
def off_of(length, M, g):
    assert g >= 1 and M % g == 0
    return length - M // g


def allowed_keys(length, M, g, ncols=None):
    """bool [M, ncols] (default: length columns): key j of row r is attended iff j <= r // g + off and j < length"""
    ncols = length if ncols is None else ncols
    lim = torch.arange(M).div(g, rounding_mode="floor") + off_of(length, M, g)
    j = torch.arange(ncols)
    return (j.view(1, -1) <= lim.view(-1, 1)) & (j.view(1, -1) < length)


def end_qb(length, M, g, qb):
    """key bound of the last row of q-block qb (<= 0: no row of it has a key)"""
    return min(length, min(128 * qb + 127, M - 1) // g + off_of(length, M, g) + 1)


def runs(length, M, g, S, qb, s):
    """does workgroup (b, h, qb, s) of a batch with ``length`` keys run?"""
    ntk = (length + 63) // 64
    tps = -(-ntk // S)
    return 64 * s * tps < end_qb(length, M, g, qb)


def qblock_count(length, M, g, S, qb):
    """the number of slots the merge reads for the rows of q-block qb"""
    e = end_qb(length, M, g, qb)
    if e <= 0:
        return 0
    ntk = (length + 63) // 64
    tps = -(-ntk // S)
    return min(-(-ntk // tps), -(-(-(-e // 64)) // tps))


# ---- the constructed-operand oracle ------------------------------------------------------------------------------------------
def _band(length, M, g, cols=None):
    m = allowed_keys(length, M, g)
    if cols is not None:
        m = m[:, cols]
    return m.view(1, 1, M, -1).expand(1, C.HQ, M, -1).contiguous()


def band_case(c, length, g):
    """the case cut to ``length`` keys with the bottom-right band of fold g as its bool mask"""
    cn = c if length == c["N"] else C.cached_subcase(c, None, length)
    return C.with_mask(cn, _band(length, c["M"], g), name=("bottom_right", g))


def split_band_cases(c, length, g, S):
    """[(s, case)] of the non-empty splits: the split's tiles of ``c`` up to ``length`` keys, with the band's columns there"""
    out = []
    for s in range(S):
        t0, t1 = split_range(length, S, s)
        if t0 >= t1:
            continue
        sub = C.cached_subcase(c, range(t0, t1), length)
        cols = torch.arange(64 * t0, min(64 * t1, length))
        out.append((s, C.with_mask(sub, _band(length, c["M"], g, cols), name=("bottom_right", g))))
    return out


def merged_bound(c, pv, length, g, S, out_dtype):
    """``constructed_cases.merged_bound`` for the band case of (length, g) under S splits -> (ref of the band case, o_bound
    [1,Hq,M,D], lse2_bound [1,Hq,M], has_key [1,Hq,M]).  Rows without a key are NaN in all three: they are held to 0 / -inf
    exactly by the caller.  Per row, only the splits in which the row keeps a key enter: W_s, B_s, L_s, the two largest L of
    rho, max |l_s| of eps and the count of additions are taken over them; a row with ONE such split has its slot merged with
    weight exp2(0) = 1 exactly (sum = 1, reciprocal 1), so its bound is that split's own, as merged_bound says of one split."""
    full = band_case(c, length, g)
    ref = C.reference64(full, pv)
    parts = split_band_cases(c, length, g, S)
    zero = torch.zeros(1, C.HQ, c["M"], dtype=torch.float64)
    W, Bs, Ls, absl, abso, part = [], [], [], [], [], []
    for _, d in parts:
        has = d["mask"].any(-1)
        r = C.reference64(d, pv)
        b_o, b_l = C.bound(d, pv, out_ulps=0)
        part.append(has)
        W.append(torch.where(has, torch.exp2(r["lse2"] - ref["lse2"]), zero).unsqueeze(-1))
        Bs.append(torch.where(has.unsqueeze(-1), b_o, zero.unsqueeze(-1)))
        Ls.append(torch.where(has, b_l, zero))
        absl.append(torch.where(has, r["lse2"].abs(), zero))
        abso.append(torch.where(has.unsqueeze(-1), r["o"].abs(), zero.unsqueeze(-1)))
    n = torch.stack(part).sum(0)
    many = n > 1
    Lst = torch.stack(Ls + [zero])  # (a zero layer: topk(2) with one split)
    top = Lst.topk(2, dim=0).values
    rho = torch.where(many, torch.exp2(top[0] + top[1]) - 1, zero).unsqueeze(-1)
    eps = torch.where(many, C._merge_eps(torch.stack(absl).amax(0)) + (n + 2) * C.U32, zero).unsqueeze(-1)
    W, Bs = torch.stack(W), torch.stack(Bs)
    wabs = (W * (torch.stack(abso) + Bs)).sum(0)
    rest = (1 + rho) * (W * Bs).sum(0) + (rho + eps) * wabs
    l_b = Lst.amax(0) + C.K_LOG2E * eps.squeeze(-1) + torch.where(many, 2 * C.U32 * ref["lse2"].abs(), zero)
    o_b = rest + 0.5 * C.out_ulp(ref["o"].abs() + rest, pv, out_dtype)
    has_key = full["mask"].any(-1)
    assert torch.equal(has_key, n > 0)
    return ref, o_b, l_b, has_key


def check(c, pv, length, g, S, o, lse, qkm, out_dtype):
    """one batch's result [1,Hq,M,D] / finished LSE [1,Hq,M] against the oracle -> (largest o ratio, largest lse ratio, rows
    without keys exactly 0 / -inf?).  Ratios over ALL elements of the rows with a key; non-finite -> inf."""
    o, lse = o.double(), lse.double()
    if length == 0:
        return 0.0, 0.0, bool((o == 0).all() and (lse == NEG_INF).all())
    ref, o_b, l2_b, has_key = merged_bound(c, pv, length, g, S, out_dtype)
    none = ~has_key
    empty_ok = bool((o[none] == 0).all() and (lse[none] == NEG_INF).all())
    if not bool(has_key.any()):
        return 0.0, 0.0, empty_ok
    lse2 = ref["lse2"][has_key]
    l_b = C.finish_bound(l2_b[has_key], lse2, qkm[has_key])
    go, gl = o[has_key], lse[has_key]
    if not (torch.isfinite(go).all() and torch.isfinite(gl).all()):
        return float("inf"), float("inf"), empty_ok
    ro = float(((go - ref["o"][has_key]).abs() / o_b[has_key]).max())
    rl = float(((gl - C.finish_lse64(lse2, qkm[has_key])).abs() / l_b).max())
    return ro, rl, empty_ok


# ---- a float64 restatement of the kernels that can make one deliberate mistake ----------------------------------------------
MISTAKES = ("diagonal_plus_one", "diagonal_minus_one", "top_left", "off_from_N", "off_not_reduced_by_split_start",
            "fold_ignored", "row_for_token", "merge_one_slot_beyond")


def restate64(c, pv, length, g, S, mistake=None, qkm=None):
    """Causal split-KV in float64 with no rounding, as the kernels are written: per workgroup (q-block, split) that runs, the
    softmax over the split's keys under the per-row limit in SPLIT-LOCAL coordinates (token + off - 64 * first tile), into a
    workspace of NaN; then the merge of the first count_qb slots of every row in split order, -inf slots dropped.
    -> (o [1,Hq,M,D], finished lse [1,Hq,M]); rows without keys 0 / -inf.  ``mistake``: one of MISTAKES."""
    M, N, D = c["M"], c["N"], c["D"]
    T = M // g
    tok = torch.arange(M) // g
    off = length - T
    if mistake == "off_from_N":
        off = N - T
    elif mistake == "top_left":
        off = 0
    elif mistake == "fold_ignored":
        tok, off = torch.arange(M), length - M
    elif mistake == "row_for_token":
        tok = torch.arange(M)
    if mistake == "diagonal_plus_one":
        off += 1
    elif mistake == "diagonal_minus_one":
        off -= 1
    t = C.logits64(c)[..., :length]
    V = C.v64(c, pv)[:, :, :length]
    nan = float("nan")
    ws_o = torch.full((S, 1, C.HQ, M, D), nan, dtype=torch.float64)
    ws_l = torch.full((S, 1, C.HQ, M), nan, dtype=torch.float64)
    nqb = (M + 127) // 128
    for s in range(S):
        t0, t1 = split_range(length, S, s)
        if t0 >= t1:
            continue
        k0, k1 = 64 * t0, min(64 * t1, length)
        for qb in range(nqb):
            if not runs(length, M, g, S, qb, s):  # (the launch rule is not among the mistakes)
                continue
            rs = slice(128 * qb, min(128 * qb + 128, M))
            lim = tok[rs] + off - (0 if mistake == "off_not_reduced_by_split_start" else k0)  # local
            ok = torch.arange(k1 - k0).view(1, -1) <= lim.view(-1, 1)
            tt = t[:, :, rs, k0:k1].masked_fill(~ok.view(1, 1, *ok.shape), NEG_INF)
            m = tt.amax(-1, keepdim=True)
            p = torch.exp2(tt - torch.where(torch.isinf(m), torch.zeros_like(m), m))
            l = p.sum(-1, keepdim=True)
            ws_o[s, :, :, rs] = (p @ V[:, :, k0:k1]) / l          # 0 / 0 = NaN for a row without a key here, as the kernel's
            ws_l[s, :, :, rs] = (m + torch.log2(l)).squeeze(-1)   # -inf there
    o = torch.zeros(1, C.HQ, M, D, dtype=torch.float64)
    lse2 = torch.full((1, C.HQ, M), NEG_INF, dtype=torch.float64)
    for qb in range(nqb):
        rs = slice(128 * qb, min(128 * qb + 128, M))
        cnt = qblock_count(length, M, g, S, qb)
        if mistake == "merge_one_slot_beyond":
            cnt = min(cnt + 1, S)
        if cnt == 0:
            continue
        l = ws_l[:cnt, :, :, rs]
        use = l != NEG_INF  # (NaN != -inf: an unwritten slot is used, and poisons the row)
        mx = torch.where(use, l, torch.full_like(l, NEG_INF)).amax(0)
        mx = torch.where(torch.isnan(l).any(0), torch.full_like(mx, nan), mx)
        w = torch.where(use, torch.exp2(l - mx), torch.zeros_like(l))
        sm = w.sum(0)
        acc = torch.where(use.unsqueeze(-1), ws_o[:cnt, :, :, rs] * w.unsqueeze(-1), torch.zeros(())).sum(0)
        some = sm > 0
        o[:, :, rs] = torch.where(some.unsqueeze(-1) | torch.isnan(sm).unsqueeze(-1), acc / sm.unsqueeze(-1), torch.zeros(()))
        lse2[:, :, rs] = torch.where(some | torch.isnan(sm), mx + torch.log2(sm), torch.full_like(mx, NEG_INF))
    lse = lse2 / math.log2(math.e) + (0 if qkm is None else qkm)
    return o, lse
