"""Constructed int8 operands and scales for the attention kernels, their fp64 reference and a DERIVED error bound.

CPU only: nothing here imports the HIP library.  tests/test_constructed_cases.py proves on the CPU that the bound is sound
(the oracle's restatement of the kernel stays inside it) and that it has teeth (a restatement with one deliberate mistake
leaves it); tests/test_constructed_logits_gpu.py holds the kernels that see every key to it, and
tests/test_constructed_subsets_gpu.py those that see a subset (block maps, key lengths, split-KV: ``subcase``, the anchored
forms for the fused-Q entry points, ``merged_bound``, ``restate_split64`` further down), and
tests/test_constructed_masks_gpu.py the attn_mask kernel under structured masks (a case may carry ``c["mask"]``: ``with_mask``,
``mask_pattern``, ``restate_mask64`` and ``public_form``), and tests/test_constructed_layouts_gpu.py the batch, head, sequence and
tile ADDRESSING: several different cases in one call, each slice held to its own case (``stack`` / ``stack_slots``, ``pack`` /
``pack_cases``, ``tile_major``, causal ``cut_case`` with M != N, their ``read_*`` / ``restate_*`` restatements and ``LAYOUT_MISTAKES``
at the end).

Every case is a dict (``case(family, variant, D, N, causal, gran)``):
  q8 [1,2,M,D] / k8 [1,1,N,D] int8; q_scale [1,2,Gq] / k_scale [1,1,Gk] fp32 in the compact layout of the granularity
  ``gran`` (oracle.sage_oracle.gid_*); q_scale_rows [1,2,M] / k_scale_cols [1,1,N] their expansions; logit_mult and the
  sm_scale that produces it; causal; v_f16 / v_bf16 [1,1,N,D]; v_f8t [1,1,D,ceil64(N)] e4m3 (tokens in NATURAL order: the
  GPU test applies quant.fp8_token_order()) with v_scale [1,1,D].
Non-causal cases have M = 150 query rows (one full 128-row q-block, one wave with 22 valid rows, waves with none);
causal cases M = N.  GQA group 2.

All scales, and logit_mult, are powers of two, so the base-2 logit of (row m, key n) is the INTEGER score S[m,n] times a
power of two: exact in fp32 and in fp64, and the same number whichever way a kernel associates the three factors.
"""
import math

import numpy as np
import torch

from oracle import sage_oracle as O

B, HQ, HK = 1, 2, 1
M_FULL = 150
LOOP_NS = (320, 384, 456, 512)  # n_fast = 4, 5, 6, 7: four-slot ring exact/+1/+2/+3, two-slot ring even/odd, ragged 456
N_ONE = 456                     # families that do not depend on the loop shape
GRANS = ("per_block", "per_warp", "per_thread")
PVS = ("fp16", "bf16", "fp8")

K_LOG2E = float(np.float32(1.4426950408889634))  # csrc/sage_common.h kLog2e
BIAS = 12582912.0                                # csrc/sage_attn_body.h kBiasF (1.5 * 2^23)
LAZY_THR = {"fp16": 6.0, "bf16": 6.0, "fp8": 3.0}  # kLazyThr
FP8_OFFSET = 8.807                               # p carries 2^(8.807 - 3) under FP8 PV (kPOff)
P_BITS = {"fp16": 11, "bf16": 8, "fp8": 4}       # significand bits of P (implicit bit included)
OUT_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp8": torch.float16}


def _pow2_logit_mult(exp=-3):
    """(sm_scale, logit_mult) with logit_mult = fp32(sm_scale) * fp32(kLog2e) == 2^exp EXACTLY in fp32: the kernels
    compute ``sm_scale * kLog2e`` in fp32 (sage_attn.hip), so such an sm_scale makes logit_mult a power of two."""
    target = np.float32(2.0 ** exp)
    x = np.float32(2.0 ** exp / 1.4426950408889634)
    for cand in (x, np.nextafter(x, np.float32(1)), np.nextafter(x, np.float32(0))):
        if np.float32(cand) * np.float32(K_LOG2E) == target:
            return float(cand), float(target)
    raise AssertionError("no fp32 sm_scale gives a power-of-two logit_mult")


SM_SCALE, LOGIT_MULT = _pow2_logit_mult(-3)


def _u(D):
    """fixed +-1 vector"""
    g = torch.Generator().manual_seed(1234 + D)
    return (torch.randint(0, 2, (D,), generator=g) * 2 - 1).to(torch.int32)


def _gid_q(M, gran):
    if gran == "per_block":
        return O.gid_per_block(M, 128)
    if gran == "per_warp":
        return O.gid_per_warp_q(M, 128, 32)
    return O.gid_per_thread_q(M, 128, 32)


def _gid_k(N, gran):
    return O.gid_per_thread_k(N) if gran == "per_thread" else O.gid_per_block(N, 64)


def _uniform_scales(M, N, gran, q_exp, k_exp):
    _, gq = _gid_q(M, gran)
    _, gk = _gid_k(N, gran)
    return torch.full((B, HQ, gq), 2.0 ** q_exp), torch.full((B, HK, gk), 2.0 ** k_exp)


def _ladder_scales(M, N, gran, q_top_exp):
    """Q: exponent q_top_exp - ((3 g + h) % 4) for group g of head h (neighbouring groups always differ);
    K: exponent ((3 g + 5 tile) % 7) - 3 in -3..3 per per-thread group g of a tile (per_block / per_warp: one per tile,
    (5 tile) % 7 - 3): neighbouring groups and neighbouring tiles always differ."""
    _, gq = _gid_q(M, gran)
    _, gk = _gid_k(N, gran)
    g = torch.arange(gq).view(1, 1, gq)
    h = torch.arange(HQ).view(1, HQ, 1)
    qs = torch.pow(2.0, (q_top_exp - ((3 * g + h) % 4)).float())
    kg = torch.arange(gk)
    if gran == "per_thread":
        ke = (3 * (kg % 4) + 5 * (kg // 4)) % 7 - 3
    else:
        ke = (5 * kg) % 7 - 3
    ks = torch.pow(2.0, ke.float()).view(1, 1, gk).expand(B, HK, gk).contiguous()
    return qs.contiguous(), ks


def _v_normal(N, D, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, HK, N, D, generator=g)
    return v


def _v_triple(v):
    """fp16, bf16 and e4m3 V^T (+ v_scale) of one real V."""
    v16 = v.to(torch.float16)
    v8t, vsc, _ = O.per_channel_fp8(v16, "HND", smooth_v=False)
    return dict(v_f16=v16, v_bf16=v.to(torch.bfloat16), v_f8t=v8t, v_scale=vsc)


def _v_big(N, D):
    """fp16 |v| in [1e4, 6e4] with alternating signs; bf16 the same pattern up to 2^16; e4m3 codes of magnitude
    256..448 (448 on every fourth key) with v_scale on the power-of-two ladder 2^(d % 7 - 3) over channels."""
    g = torch.Generator().manual_seed(77)
    sign = 1.0 - 2.0 * ((torch.arange(N).view(N, 1) + torch.arange(D).view(1, D)) % 2)
    mag = 1.0e4 + 5.0e4 * torch.rand(N, D, generator=g)
    mag[::4] = 6.0e4
    v16 = (sign * mag).view(B, HK, N, D).to(torch.float16)
    vbf = (sign * mag * (65536.0 / 6.0e4)).view(B, HK, N, D).to(torch.bfloat16)
    codes = torch.tensor([448.0, 256.0, 320.0, 416.0])[torch.arange(N) % 4].view(N, 1) * sign  # all exact in e4m3
    npad = O.cdiv(N, 64) * 64
    v8t = torch.zeros(B, HK, D, npad)
    v8t[..., :N] = codes.t()
    vsc = torch.pow(2.0, (torch.arange(D) % 7 - 3).float()).view(B, HK, D).contiguous()
    return dict(v_f16=v16, v_bf16=vbf, v_f8t=v8t.to(torch.float8_e4m3fn), v_scale=vsc)


def regran(c, gran):
    """The same case with its (uniform) scales laid out for another granularity: the logits do not change, so the copy
    shares the cached reference."""
    assert c["family"] in ("ramp", "extreme_s", "one_hot")
    d = dict(c)
    _, gq = _gid_q(c["M"], gran)
    _, gk = _gid_k(c["N"], gran)
    d["q_scale"] = c["q_scale"][..., :1].expand(B, HQ, gq).contiguous()
    d["k_scale"] = c["k_scale"][..., :1].expand(B, HK, gk).contiguous()
    d["gran"] = gran
    assert torch.equal(O.expand_q_scale(d["q_scale"], c["M"], gran), c["q_scale_rows"])
    return d


def _finish(c, M, N, gran):
    c["_cache"] = {}
    c["q_scale_rows"] = O.expand_q_scale(c["q_scale"], M, gran)
    c["k_scale_cols"] = O.expand_k_scale(c["k_scale"], N, gran)
    c.update(M=M, N=N, gran=gran, logit_mult=LOGIT_MULT, sm_scale=SM_SCALE)
    assert c["q8"].dtype == torch.int8 and c["k8"].dtype == torch.int8
    return c


def cached_subcase(c, tiles=None, length=None):
    """subcase, kept in the cache of ``c`` (shared by its regran copies, whose logits are the same): for callers that only
    READ the result"""
    key = ("sub", None if tiles is None else tuple(tiles), length)
    cache = c.setdefault("_cache", {})
    if key not in cache:
        cache[key] = subcase(c, tiles, length)
    return cache[key]


def _anchor_scales(c):
    """Move powers of two from k_scale into q_scale until the smallest q_scale is 2^1; every product stays what it was."""
    shift = 2.0 ** (1 - int(torch.log2(c["q_scale"].min())))
    for key, f in (("q_scale", shift), ("q_scale_rows", shift), ("k_scale", 1 / shift), ("k_scale_cols", 1 / shift)):
        c[key] = c[key] * f
    assert float(torch.log2(c["q_scale"]).min()) == 1.0 and torch.equal(torch.log2(c["q_scale"]), torch.log2(c["q_scale"]).round())
    assert torch.equal(c["q8"][..., -1], torch.full_like(c["q8"][..., -1], 127)) and not c["k8"][..., -1].any()
    c["anchored"], c["_cache"] = True, {}
    return c


def anchor(c):
    """The ANCHORED form of a case, for the entry points that quantize Q themselves (fused Q): head-dim channel D - 1 is
    reserved, k8 = 0 there for every key and q8 = 127 there for every row, so that every quantization group of Q = q8 * 2^e
    has amax 127 * 2^e and the quantizer must return q8 and 2^e exactly (``q_real``; tests/test_constructed_cases.py asserts it
    through the oracle's quantizers).  The per-thread numerics add 1e-7 to the scale, which fp32 absorbs only for e >= 1: the
    q scales are moved up to 2^1 and above and k_scale, which the entry point is handed directly, absorbs the rest.  The
    overwritten channel changes the scores (a rank-one family keeps its form with D - 1 in the place of D); the reference is
    computed from the operands, as always.  ``ramp`` and ``offset`` build their anchored form themselves (their channel 0
    carries the remainder digit)."""
    assert c["family"] not in ("ramp", "offset") and c["gran"] != "per_block" and not c.get("anchored")
    d = dict(c)
    d["q8"], d["k8"] = c["q8"].clone(), c["k8"].clone()
    d["q8"][..., -1] = 127
    d["k8"][..., -1] = 0
    return _anchor_scales(d)


def q_real(c, dtype):
    """Q = q8 * 2^e of an anchored case in fp16 / bf16, exact (|q8| <= 127 has 7 bits, 2^e is in range)"""
    assert c.get("anchored")
    q = c["q8"].float() * c["q_scale_rows"].unsqueeze(-1)
    assert torch.equal(q.to(dtype).float(), q)
    return q.to(dtype)


def subcase(c, tiles=None, length=None):
    """The case restricted to the listed 64-key tiles of ``c`` (default: all), the list clipped to the first ``length`` keys
    (default: N) so that its last tile may be ragged: again an ordinary case -- k8, k_scale_cols and the three V gathered (the
    e4m3 V^T zero-padded to a multiple of 64), the new N -- on which scores, scale_matrix, reference64, bound, ratios, oracle
    and restate64 work unchanged.  Only the LAST tile of a case can be ragged and the list ascends, so the tiles of the
    subcase are again whole except the last.  Causal is kept for prefix subsets only (the ``length`` form), where ``allowed``
    stays correct: key n of the subcase is key n of the case.  The compact q_scale is kept, the compact k_scale dropped:
    what a kernel is handed are the operands of ``c``."""
    N = c["N"]
    length = N if length is None else max(0, min(int(length), N))
    ntk = O.cdiv(length, 64)
    tiles = list(range(ntk)) if tiles is None else [int(t) for t in tiles if t < ntk]
    assert tiles == sorted(set(tiles)) and len(tiles) > 0, "an empty subset has no softmax"
    prefix = tiles == list(range(len(tiles)))
    assert prefix or not c["causal"], "a causal case keeps its meaning under a prefix only"
    idx = torch.cat([torch.arange(64 * t, min(64 * t + 64, length)) for t in tiles])
    n = idx.numel()
    d = {k: v for k, v in c.items() if k not in ("k_scale", "_cache")}
    d["_cache"] = {}
    d["k8"], d["k_scale_cols"] = c["k8"][:, :, idx].contiguous(), c["k_scale_cols"][:, :, idx].contiguous()
    d["v_f16"], d["v_bf16"] = c["v_f16"][:, :, idx].contiguous(), c["v_bf16"][:, :, idx].contiguous()
    v8 = torch.zeros(B, HK, c["D"], O.cdiv(n, 64) * 64, dtype=torch.uint8)
    v8[..., :n] = c["v_f8t"].view(torch.uint8)[..., idx]
    d["v_f8t"] = v8.view(torch.float8_e4m3fn)
    d.update(N=n, tiles=tuple(tiles), length=length)
    return d


# ---------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------

def _ladder_operands(D, N, M, gran, q_top_exp):
    gq = torch.Generator().manual_seed(100 + D)
    q8 = torch.randint(-127, 128, (B, HQ, 512, D), generator=gq)[:, :, :M].to(torch.int8)
    gk = torch.Generator().manual_seed(200 + D)
    k_real = 48.0 * torch.randn(B, HK, 512, D, generator=gk)[:, :, :N]
    qs, ks = _ladder_scales(M, N, gran, q_top_exp)
    kcols = O.expand_k_scale(ks, N, gran)
    k8 = torch.round(k_real / kcols.unsqueeze(-1)).clamp(-127, 127).to(torch.int8)
    return dict(q8=q8.contiguous(), k8=k8.contiguous(), q_scale=qs, k_scale=ks)


def scale_ladder(D, N, causal, gran, lsb_exp=-12, big_v=False):
    """A seeded real K (sigma 48) quantized with hand-chosen power-of-two scales 2^-3..2^3, permuted over the per-thread key
    groups and over the tiles (coarse scales use a few integer levels, fine ones clamp at +-127); uniform int8 Q with
    per-row-group scales on a ladder of four exponents.  The LARGEST LSB of any row, q_scale * logit_mult * 2^3, is
    2^lsb_exp: -12 for the ordinary family, -6 / -5 / -4 for ``coarse_lsb``."""
    M = N if causal else M_FULL
    c = _ladder_operands(D, N, M, gran, lsb_exp)  # top q_scale 2^lsb_exp: times logit_mult 2^-3 and the top k_scale 2^3
    c.update(_v_big(N, D) if big_v else _v_triple(_v_normal(N, D, 300 + D)))
    c.update(family="big_v" if big_v else ("scale_ladder" if lsb_exp == -12 else "coarse_lsb"), causal=causal, D=D)
    return _finish(c, M, N, gran)


RAMP_UNITS = {  # step of the steepest row's per-tile maximum, in units of 2^-10 (base-2 logits)
    "0.5": 512, "6-": 6 * 1024 - 1, "6": 6 * 1024, "6+": 6 * 1024 + 1, "3-": 3 * 1024 - 1, "3": 3 * 1024,
    "3+": 3 * 1024 + 1, "40": 40 * 1024}
RAMP_R = (4, -4, 2, -2, 1, -1, 0)  # r_m cycles with period 7: every 32-row wave holds every trend, both signs
RAMP_SHAPES = ("ascending", "descending", "sawtooth")


def ramp_steps(pv):
    t = "6" if pv != "fp8" else "3"
    return ("0.5", t + "-", t, t + "+", "40")


def _ramp_levels(shape, ntiles):
    if shape == "ascending":
        lv = list(range(ntiles))
    elif shape == "descending":
        lv = list(range(ntiles - 1, -1, -1))
    elif shape == "peak":  # 0 2 4 6 7 5 3 1: the maximum in the MIDDLE (split-KV: the dominant split is a middle one)
        lv = [2 * j if 2 * j < ntiles else 2 * (ntiles - 1 - j) + 1 for j in range(ntiles)]
    else:  # 0 1 0 2 1 3 2 4: the maximum grows by one step on every odd tile, a tile two steps below it follows
        lv = [(j + 1) // 2 if j % 2 else max(j // 2 - 1, 0) for j in range(ntiles)]
    return [x - 3 for x in lv]  # centred so that |K| stays inside the digits' range


def _rank_one(D, M, N, r, K, anchor):
    """q8 [1,Hq,M,D], k8 [1,1,N,D] with q.k = r_m * K_n exactly (see ``ramp``).  ``anchor``: the digits use D - 1 channels and
    the last channel is the anchor of ``anchor()``: q8 = 127, k8 = 0."""
    Dd = D - 1 if anchor else D
    u = _u(D)[:Dd]
    w = torch.full((Dd,), 31, dtype=torch.int32)
    w[0] = 1
    q8 = (r.view(M, 1) * (w * u).view(1, Dd)).view(1, 1, M, Dd).expand(B, HQ, M, Dd)
    A = torch.round(K.double() / 31).to(torch.int64)
    rem = K - 31 * A
    base = torch.div(A, Dd - 1, rounding_mode="floor")
    extra = A - base * (Dd - 1)  # 0 .. Dd-2
    dig = base.view(N, 1) + (torch.arange(Dd - 1).view(1, Dd - 1) < extra.view(N, 1)).to(torch.int64)
    digits = torch.cat([rem.view(N, 1), dig], dim=1)
    assert digits.abs().max() <= 127 and (q8.abs().max() <= 127)
    k8 = (digits.to(torch.int32) * u.view(1, Dd)).view(B, HK, N, Dd)
    if anchor:
        q8 = torch.cat([q8, torch.full((B, HQ, M, 1), 127, dtype=q8.dtype)], dim=-1)
        k8 = torch.cat([k8, torch.zeros(B, HK, N, 1, dtype=k8.dtype)], dim=-1)
    return q8.to(torch.int8).contiguous(), k8.to(torch.int8).contiguous()


def ramp(D, N, causal, gran, step="6", shape="ascending", anchor=False):
    """Rank-one integer scores S[m,n] = r_m * K_n, known in closed form.

    q8[m,:] = r_m * w * u and k8[n,:] = digits(K_n) * u with u a fixed +-1 vector and w = (1, 31, 31, ..., 31), so that
    q.k = r_m * (digit_0 + 31 * sum(other digits)) = r_m * K_n for ANY integer |K_n| <= 31*127*(D-1): the plain form
    r_m*u, c_n*u reaches only products of two int8, and the steps thr -+ 2^-10 need the 13-bit primes 6143 / 3071 (and
    5*1229, 7*439) as a factor.  K_n is a staircase over the 64-key tiles, K = level(tile) * units, r_m cycles through
    (4,-4,2,-2,1,-1,0) inside every wave.  With q_scale * k_scale * logit_mult = 2^-12 the steepest rows (r = 4) see their
    tile maximum move by exactly units * 2^-10 per level.  ``anchor``: the anchored form (``anchor()``), one digit channel
    fewer."""
    M = N if causal else M_FULL
    units = RAMP_UNITS[step]
    r = torch.tensor([RAMP_R[m % 7] for m in range(M)], dtype=torch.int32)
    ntiles = O.cdiv(N, 64)
    K = torch.tensor(_ramp_levels(shape, ntiles), dtype=torch.int64).repeat_interleave(64)[:N] * units
    q8, k8 = _rank_one(D, M, N, r, K, anchor)
    qs, ks = _uniform_scales(M, N, gran, -5, -4)  # 2^-5 * 2^-4 * 2^-3 = 2^-12
    c = dict(q8=q8, k8=k8, q_scale=qs, k_scale=ks, family="ramp", causal=causal, D=D, r=r, K=K, units=units)
    c.update(_v_triple(_v_normal(N, D, 400 + D)))
    c = _finish(c, M, N, gran)
    return _anchor_scales(c) if anchor else c


OFFSET_LEVEL = 140000  # * 2^-7: every logit of a row with r = +-1 is about +-1094 (base 2)


def offset(D, N, gran):
    """Anchored rank-one scores with a LARGE COMMON LEVEL and a coarser LSB (2^-7): K_n = 140000 + level(tile) + n % 3 (the
    sawtooth levels, -3..4), r_m cycling through (4,-4,2,-2,1,-1) -- no zero row.  Every row's logits are |r| * 1094 or more in
    magnitude while they differ by at most 4 * 9 * 2^-7 = 0.28 along the row: the LSEs of any two splits of equal key count
    lie within 0.28 of each other, at 2^10 .. 2^12.  A merge that exponentiates before subtracting the maximum overflows or
    returns 0 / 0, and the finish mx + log2(sum) rounds at 2^-13 .. 2^-11 absolute.  delta of ``bound`` is 0.75 * 2^-7 +
    2^-24 * Smax * 2^-7 < 2^-6."""
    M = M_FULL
    r = torch.tensor([(4, -4, 2, -2, 1, -1)[m % 6] for m in range(M)], dtype=torch.int32)
    n = torch.arange(N, dtype=torch.int64)
    lv = torch.tensor(_ramp_levels("sawtooth", O.cdiv(N, 64)), dtype=torch.int64).repeat_interleave(64)[:N]
    K = OFFSET_LEVEL + lv + n % 3
    q8, k8 = _rank_one(D, M, N, r, K, True)
    qs, ks = _uniform_scales(M, N, gran, 0, -4)  # 2^0 * 2^-4 * 2^-3 = 2^-7
    c = dict(q8=q8, k8=k8, q_scale=qs, k_scale=ks, family="offset", causal=False, D=D, r=r, K=K)
    c.update(_v_triple(_v_normal(N, D, 450 + D)))
    return _anchor_scales(_finish(c, M, N, gran))


def extreme_s(D, N, causal, gran, variant="corner"):
    """corner: every q8 = -128, k8 alternating -128 / 127 by key: S = +D*2^14 (2^21 at head_dim 128, the largest score the
    int8 format can produce) and -D*128*127 side by side in one tile; the scale product 2^-18 (2^-17 at head_dim 64) makes
    the logit spread 15.9.  zero: q8 = 0 and random k8: uniform weights, o = mean of V, lse2 = log2(keys)."""
    M = N if causal else M_FULL
    if variant == "corner":
        q8 = torch.full((B, HQ, M, D), -128, dtype=torch.int8)
        kv = torch.where(torch.arange(N) % 2 == 0, -128, 127).view(1, 1, N, 1).expand(B, HK, N, D)
        k8 = kv.to(torch.int8).contiguous()
        qs, ks = _uniform_scales(M, N, gran, -8 if D == 128 else -7, -7)  # * 2^-3 -> 2^-18 / 2^-17
    else:
        q8 = torch.zeros(B, HQ, M, D, dtype=torch.int8)
        k8 = torch.randint(-127, 128, (B, HK, N, D), generator=torch.Generator().manual_seed(500 + D)).to(torch.int8)
        qs, ks = _uniform_scales(M, N, gran, -5, -4)
    c = dict(q8=q8, k8=k8, q_scale=qs, k_scale=ks, family="extreme_s", variant=variant, causal=causal, D=D)
    c.update(_v_triple(_v_normal(N, D, 600 + D)))
    return _finish(c, M, N, gran)


ONE_HOT_KEYS = ("first", "63", "ragged", "last")


def one_hot_key(N, where):
    if isinstance(where, int):
        return where
    return {"first": 0, "63": 63, "ragged": 64 * (N // 64), "last": N - 1}[where]


def one_hot(D, N, causal, gran, where="last", subnormal=False):
    """Rank-one r_m*u, c_n*u with one key far ahead.  Ordinary: c_hot = 127, the others in -2..2, r_m in 40..127, LSB 2^-12:
    the lead D*r_m*(127-2)*2^-12 is >= 78 (base 2).  subnormal: the others are c = 0, c_hot = 4096/D and r_m cycles through
    15..24, so every other key has p = 2^-r_m relative to the hot one: inside fp16's subnormal range (2^-15..2^-24)."""
    M = N if causal else M_FULL
    u = _u(D)
    hot = one_hot_key(N, where)
    if subnormal:
        r = torch.tensor([15 + m % 10 for m in range(M)], dtype=torch.int32)
        cn = torch.zeros(N, dtype=torch.int32)
        cn[hot] = 4096 // D
    else:
        r = torch.tensor([40 + (m * 37) % 88 for m in range(M)], dtype=torch.int32)
        cn = torch.randint(-2, 3, (N,), generator=torch.Generator().manual_seed(700)).to(torch.int32)
        cn[hot] = 127
    q8 = (r.view(M, 1) * u.view(1, D)).view(1, 1, M, D).expand(B, HQ, M, D).to(torch.int8).contiguous()
    k8 = (cn.view(N, 1) * u.view(1, D)).view(B, HK, N, D).to(torch.int8).contiguous()
    qs, ks = _uniform_scales(M, N, gran, -5, -4)
    c = dict(q8=q8, k8=k8, q_scale=qs, k_scale=ks, family="one_hot", causal=causal, D=D, hot=hot, r=r, cn=cn,
             subnormal=subnormal)
    c.update(_v_triple(_v_normal(N, D, 800 + D)))
    return _finish(c, M, N, gran)


def coarse_lsb(D, N, causal, gran, lsb_exp=-6):
    return scale_ladder(D, N, causal, gran, lsb_exp=lsb_exp)


def big_v(D, N, causal, gran):
    return scale_ladder(D, N, causal, gran, big_v=True)


# ---------------------------------------------------------------------------------------------------------------------
# fp64 reference
# ---------------------------------------------------------------------------------------------------------------------

def scores(c):
    """exact integer scores [1,Hq,M,N] as float64 (|S| <= 2^21)"""
    g = HQ // HK
    return c["q8"].double() @ c["k8"].double().repeat_interleave(g, dim=1).transpose(2, 3)


def scale_matrix(c, q_rows=None, k_cols=None):
    """fp32 q_scale*logit_mult times k_scale as the kernels form it (body.h: qsc = q_scale * logit_mult, sc = qsc * k), in
    float64.  With the power-of-two scales of this file every product is exact."""
    q_rows = c["q_scale_rows"] if q_rows is None else q_rows
    k_cols = c["k_scale_cols"] if k_cols is None else k_cols
    qsc = q_rows * torch.tensor(c["logit_mult"], dtype=torch.float32)
    sc = qsc.unsqueeze(-1) * k_cols.repeat_interleave(HQ // HK, dim=1).unsqueeze(2)
    return sc.double()


def additive(c):
    """the additive attn_mask of the case in float64 [Bm,Hq,M,N], or None (no mask, a bool mask)"""
    mask = c.get("mask")
    return None if mask is None or mask.dtype == torch.bool else mask.double()


def logits64(c):
    """base-2 logits t = S * scale (+ the additive attn_mask) in float64, nothing masked out yet"""
    t, add = scores(c) * scale_matrix(c), additive(c)
    return t if add is None else t + add


def allowed(c, M=None, N=None):
    """the keys each row attends: [1,1,M,N], or [Bm,Hq,M,N] under ``c["mask"]`` -- a bool mask itself, the keys of an additive
    mask whose term is not -inf"""
    M, N = c["M"] if M is None else M, c["N"] if N is None else N
    mask = c.get("mask")
    if mask is not None:
        assert not c["causal"] and tuple(mask.shape[1:]) == (HQ, M, N), "attn_mask: non-causal, [Bm,Hq,M,N]"
        return mask.clone() if mask.dtype == torch.bool else mask.float() > float("-inf")
    if c["causal"]:
        return (torch.arange(N).view(1, 1, 1, N) <= torch.arange(M).view(1, 1, M, 1))
    return torch.ones(1, 1, M, N, dtype=torch.bool)


def v64(c, pv):
    """the V a kernel multiplies, dequantised, float64 [1,Hq,N,D]"""
    if pv == "fp16":
        v = c["v_f16"].double()
    elif pv == "bf16":
        v = c["v_bf16"].double()
    else:
        v = (c["v_f8t"].float().double()[..., :c["N"]] * c["v_scale"].double().unsqueeze(-1)).transpose(2, 3)
    return v.repeat_interleave(HQ // HK, dim=1)


def reference64(c, pv):
    """fp64 softmax (base 2) of the dequantised integers times the dequantised V.
    -> dict(o [1,Hq,M,D], lse2 [1,Hq,M], W normalised weights [1,Hq,M,N], wabsv = W @ |V|, sumabsv = sum_j |V_jd| over the
    keys the row attends).  Under ``c["mask"]`` [Bm,Hq,M,N] every result has Bm batch slices (the operands are the same, the
    masks differ); an additive mask is added to t in float64 before the softmax.  A row that keeps no key is NaN."""
    key, cache = ("ref", pv), c.setdefault("_cache", {})
    if key in cache:
        return cache[key]
    t = logits64(c)
    ok = allowed(c)
    t = t.masked_fill(~ok, float("-inf"))
    m = t.amax(-1, keepdim=True)
    p = torch.exp2(t - m)
    l = p.sum(-1, keepdim=True)
    W = p / l
    V = v64(c, pv)
    out = dict(o=W @ V, lse2=(m + torch.log2(l)).squeeze(-1), W=W, wabsv=W @ V.abs(),
               sumabsv=ok.double().expand(-1, HQ, -1, -1) @ V.abs())
    cache[key] = out
    return out


def _ulp(x, mant, emin):
    e = torch.floor(torch.log2(x.abs())).clamp(min=emin)
    return torch.exp2(e - mant)


def out_ulp(x, pv, dtype=None):
    """spacing of the output dtype at |x| (fp16 for fp16 / fp8 PV, bf16 for bf16 PV), subnormal floor included"""
    return _ulp(x, 10, -14) if (dtype or OUT_DTYPE[pv]) == torch.float16 else _ulp(x, 7, -126)


def row_lsb(c):
    """largest LSB of each row: max over the attended keys of q_scale * logit_mult * k_scale, [1,Hq,M] float64"""
    sc = scale_matrix(c).masked_fill(~allowed(c), 0.0)
    return sc.amax(-1)


def bound(c, pv, D=None, delta_zero=False, out_ulps=2):
    """Per-element tolerance of a kernel's (o, lse2) against reference64 -> (o_bound [1,Hq,M,D], lse_bound [1,Hq,M]).

    Every number is a format width or a constant of csrc/sage_attn_body.h:

      |o - o64|       <= (2 * 2^-t + (2^(2 delta) - 1) + 2^-18) * (W @ |V|)  +  sub  +  2 output ulps of |o64|
      |lse2 - lse2_64| <= [log2(1 + 2^-11) if D = 64 and fp16 P] + delta + 1.4427 * N * 2^-24 + 2 fp32 ulps of |lse2_64|

    * 2^-t, t = 11 / 8 / 4 significand bits of P in fp16 / bf16 / e4m3: one RNE rounding of every p is within 2^-t
      relative of it (half an ulp of a t-bit significand is at most 2^-t of the value).  A second 2^-t because the FP16-PV
      kernel at head_dim 64 divides by the sum of the ROUNDED P (row-sum MFMA): numerator and denominator each move by
      2^-t relative.  (For e4m3 this is the hard form 2^-3 of tests/test_fp8_derived_bound.py; its 6-sigma form assumes
      many comparable keys and does not hold for rows that a few keys dominate.)
    * delta = (12582912 + Smax) * 2^-24 * s with s the row's largest LSB and Smax the largest |S| of the case.  The
      kernel evaluates p = exp2(fma(as_float(bias + S), sc, c0)) with c0 = fma(-12582912, sc, kPOff - m_run), m_run the
      logit of some score: |c0| <= (12582912 + Smax) * sc (+ kPOff) and its rounding is half an ulp, 2^-24 |c0|.  One
      tile's exponent is therefore off by up to delta, the same for all its keys, and two tiles may err in opposite
      directions: weights move by 2^(2 delta) - 1 relative to each other.  At Smax = 2^21 delta is 0.875 s, not the
      0.75 s the comments in the kernel and in tests/conftest.py state (0.75 is its value for Smax << 12582912).
      FP8 PV adds the rounding of (kPOff - m_run) itself, which is exact only for kPOff = 0: half an ulp of at most
      Smax * s + 8.807, i.e. 2^-24 * (Smax * s + 8.807) more.
    * 2^-18 covers v_exp_f32 (1 ulp, 2^-23), the rounding of the fma result (|exponent| <= 31 for any p that survives
      fp16: 2^-24 * 31 * ln 2) and the fp32 accumulation over <= 512 keys.
    * sub, the subnormal floor of P: an fp16 P below 2^-14 is rounded to a multiple of 2^-24, off by <= 2^-25 absolute,
      while the row's largest p is >= 1 so l >= 1: 2^-25 * sum_j |V_jd| over the row's keys.  bf16 has fp32's exponent
      range: 0.  e4m3: half the subnormal spacing 2^-9 is 2^-10, and the row's largest p is at least 2^(8.807 - 3) (the
      running maximum lags the true one by at most kLazyThr = 3): 2^-10 * 2^-5.807 * sum_j |V_jd|.
    * 2 output ulps: the final rounding to fp16 / bf16 is half an ulp; the second guards the ulp boundary between o and
      o64.
    LSE: log2(1 + 2^-11) is the relative error of a sum of fp16-rounded P (conftest.LSE2_TOL_ROUNDED_P's first term);
    delta moves l by 2^(+-delta); N fp32 additions of positive terms each lose <= 2^-24 relative, log2(e) * N * 2^-24 in
    the logarithm (v_log_f32's own ulp is inside the 2 fp32 ulps).
    * attn_mask (``c["mask"]``; sage_attn_body.h, the HAS_MASK loop).  A bool mask needs no new term: a masked score is the bit
      pattern of -inf, p = exp2(fma(-inf, sc, c0)) is exactly 0, and the keys a row keeps go through the arithmetic above;
      ``allowed`` (hence sumabsv, the row LSB) follows the mask.  An ADDITIVE mask adds to delta
          2^-24 * (Tmax + 3 * Umax),
      Tmax the row's largest |t| and Umax its largest |t + mask| over the keys it keeps (term not -inf).  The kernel
      (to_float_logits, then the MASKED && fmask branch of prob) forms, in this order, t32 = fl(fma(as_float(bias + S), sc,
      -bias * sc)), u = fl(t32 + mask) and fl(u - m_run) (+ kPOff = 0: the operator has no FP8 PV): three roundings of half an
      ulp of their results, 2^-24 |t|, 2^-24 |u| and 2^-24 |u - m_run| <= 2^-24 * 2 Umax, since m_run is itself some u of the
      row.  (The c0 of the bullet above is not formed on this path; its term is kept, so one delta holds for both.)  The sum
      enters rel and the LSE bound as delta does.  A key at -inf has u = -inf and p = 0 exactly.
    ``delta_zero``: for operands whose logits are all equal on a row no relative movement between tiles can change the
    weights' ratios -- used by the degenerate-input operator tests, where the issue sets delta = 0.
    ``out_ulps``: 0 for a result that is stored in fp32 (the split-KV partials in the workspace)."""
    D = c["D"] if D is None else D
    ref = reference64(c, pv)
    t = P_BITS[pv]
    smax = float(scores(c).abs().max())
    s = row_lsb(c)
    delta = (BIAS + smax) * 2.0 ** -24 * s
    if pv == "fp8":
        delta = delta + 2.0 ** -24 * (smax * s + FP8_OFFSET)
    add = additive(c)
    if add is not None:
        ok, tl = allowed(c), scores(c) * scale_matrix(c)
        tmax = tl.abs().expand_as(ok).masked_fill(~ok, 0.0).amax(-1)
        umax = (tl + add).abs().masked_fill(~ok, 0.0).amax(-1)
        delta = delta + 2.0 ** -24 * (tmax + 3 * umax)
    if delta_zero:
        delta = torch.zeros_like(delta)
    rel = 2 * 2.0 ** -t + (torch.exp2(2 * delta) - 1) + 2.0 ** -18
    if pv == "fp16":
        sub = 2.0 ** -25 * ref["sumabsv"]
    elif pv == "bf16":
        sub = torch.zeros_like(ref["sumabsv"])
    else:
        sub = 2.0 ** -10 * 2.0 ** -(FP8_OFFSET - 3.0) * ref["sumabsv"]
    o_b = rel.unsqueeze(-1) * ref["wabsv"] + sub + out_ulps * out_ulp(ref["o"], pv, c.get("out_dtype"))
    l_b = delta + K_LOG2E * c["N"] * 2.0 ** -24 + 2 * _ulp(ref["lse2"], 23, -126)
    if D == 64 and pv == "fp16":
        l_b = l_b + math.log2(1 + 2.0 ** -11)
    return o_b, l_b


def ratio_tensors(c, pv, o, lse2, out_ulps=2):
    """|o - o64| / bound [1,Hq,M,D] and |lse2 - lse2_64| / bound [1,Hq,M], element by element; non-finite -> inf"""
    ref = reference64(c, pv)
    o_b, l_b = bound(c, pv, out_ulps=out_ulps)
    inf = torch.tensor(float("inf"), dtype=torch.float64)
    o, lse2 = o.double(), lse2.double()
    return (torch.where(torch.isfinite(o), (o - ref["o"]).abs() / o_b, inf),
            torch.where(torch.isfinite(lse2), (lse2 - ref["lse2"]).abs() / l_b, inf))


def ratios(c, pv, o, lse2):
    """largest |o - o64| / bound and |lse2 - lse2_64| / bound over ALL elements (no percentile); non-finite -> inf"""
    ref = reference64(c, pv)
    o_b, l_b = bound(c, pv)
    o, lse2 = o.double(), lse2.double()
    if not (torch.isfinite(o).all() and torch.isfinite(lse2).all()):
        return float("inf"), float("inf")
    return float(((o - ref["o"]).abs() / o_b).max()), float(((lse2 - ref["lse2"]).abs() / l_b).max())


# ---------------------------------------------------------------------------------------------------------------------
# the oracle on a case, and a float64 restatement of the kernel's loop that can make one deliberate mistake
# ---------------------------------------------------------------------------------------------------------------------

def v_of(c, pv):
    return {"fp16": c["v_f16"], "bf16": c["v_bf16"], "fp8": c["v_f8t"]}[pv]


def oracle(c, pv):
    """oracle.sage_oracle.attn_tile_loop, "hip" flavour, on the case -> (o in the output dtype, lse2 fp32)"""
    key, cache = ("oracle", pv), c.setdefault("_cache", {})
    if key not in cache:
        mask = c.get("mask")
        rep = (lambda t: t) if mask is None else (lambda t: t.expand(mask.shape[0], *t.shape[1:]))
        cache[key] = O.attn_tile_loop(rep(c["q8"]), rep(c["k8"]), rep(v_of(c, pv)), rep(c["q_scale_rows"]),
                                  rep(c["k_scale_cols"]), logit_mult=c["logit_mult"], is_causal=c["causal"],
                                  pv="fp8" if pv == "fp8" else "fp16", v_scale=c["v_scale"] if pv == "fp8" else None,
                                  out_dtype=OUT_DTYPE[pv], flavor="hip", attn_mask=mask)
    return cache[key]


MISTAKES = ("swap_key_groups", "tile3_scales_of_tile2", "q_group_xor_1", "drop_last_key", "admit_key_N", "wrap_2_21",
            "clamp_p_2_5")


def restate64(c, pv, mistake=None):
    """The kernel's loop in float64 with NO rounding: 64-key tiles, a running maximum that is raised only when some row of
    the 32-row wave sees its tile maximum exceed m_run + kLazyThr (the wave-wide ballot), p = 2^(t - m_run).  Without a
    mistake it equals reference64 to float64 accuracy; ``mistake`` makes exactly one of MISTAKES."""
    M, N, gran = c["M"], c["N"], c["gran"]
    S = scores(c)
    q_rows, k_cols = c["q_scale_rows"], c["k_scale_cols"]
    V = v64(c, pv)
    ok = allowed(c).expand(1, HQ, M, N).clone()
    if mistake == "swap_key_groups":      # key groups 0/1 and 2/3 of every tile take each other's scale
        n = torch.arange(N)
        partner = torch.where(((n % 8) // 2) % 2 == 0, n + 2, n - 2).clamp(max=N - 1)
        k_cols = k_cols[:, :, partner]
    elif mistake == "tile3_scales_of_tile2":
        k_cols = k_cols.clone()
        k_cols[:, :, 192:256] = c["k_scale_cols"][:, :, 128:192]
    elif mistake == "q_group_xor_1":
        gid, ng = _gid_q(M, gran)
        q_rows = c["q_scale"][:, :, (gid ^ 1).clamp(max=ng - 1)]
    elif mistake == "drop_last_key":
        ok[..., N - 1] = False
    elif mistake == "admit_key_N":        # the zero padding after the last key: S = 0, V = 0, seen by every row
        S = torch.cat([S, torch.zeros(1, HQ, M, 1, dtype=S.dtype)], dim=-1)
        k_cols = torch.cat([k_cols, k_cols[:, :, -1:]], dim=-1)
        V = torch.cat([V, torch.zeros(1, HQ, 1, V.shape[-1], dtype=V.dtype)], dim=2)
        ok = torch.cat([ok, torch.ones(1, HQ, M, 1, dtype=torch.bool)], dim=-1)
    elif mistake == "wrap_2_21":          # a 22-bit accumulator: +2^21 becomes -2^21
        S = torch.remainder(S + 2.0 ** 21, 2.0 ** 22) - 2.0 ** 21
    t_all = (S * scale_matrix(c, q_rows, k_cols)).masked_fill(~ok, float("-inf"))
    return _lazy_loop64(t_all, V, pv, clamp=32.0 if mistake == "clamp_p_2_5" else None)


def _lazy_loop64(t_all, V, pv, clamp=None):
    """the tile loop of restate64 on the float64 logits t_all [..,Hq,M,N] (-inf = not attended) -> (o, lse2)"""
    M = t_all.shape[-2]
    thr = LAZY_THR[pv]
    NEG = float("-inf")
    m_run = torch.full(t_all.shape[:-1], NEG, dtype=torch.float64)
    l = torch.zeros(t_all.shape[:-1], dtype=torch.float64)
    acc = torch.zeros(t_all.shape[:-1] + (V.shape[-1],), dtype=torch.float64)
    wave = torch.arange(M) // 32
    nw = int(wave.max()) + 1
    for n0 in range(0, t_all.shape[-1], 64):
        t = t_all[..., n0:n0 + 64]
        mx = t.amax(-1)
        need = (mx > m_run + thr) | (torch.isinf(m_run) & ~torch.isinf(mx))
        wave_need = torch.stack([need[..., wave == w].any(-1) for w in range(nw)], dim=-1)
        do = wave_need[..., wave]
        m_new = torch.where(do, torch.maximum(m_run, mx), m_run)
        alpha = torch.where(torch.isinf(m_new), torch.ones_like(m_new),
                            torch.exp2(torch.where(torch.isinf(m_run), torch.full_like(m_run, NEG), m_run - m_new)))
        safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        p = torch.exp2(t - safe.unsqueeze(-1))
        if clamp is not None:
            p = p.clamp(max=clamp)
        l = l * alpha + p.sum(-1)
        acc = acc * alpha.unsqueeze(-1) + p @ V[:, :, n0:n0 + 64]
        m_run = m_new
    return acc / l.unsqueeze(-1), m_run + torch.log2(l)


# ---------------------------------------------------------------------------------------------------------------------
# which cases each family spans (shared by the CPU soundness test and the GPU test)
# ---------------------------------------------------------------------------------------------------------------------

FAMILIES = ("scale_ladder", "ramp", "extreme_s", "one_hot", "coarse_lsb", "big_v")


def family_cases(family, D, pv, grans=GRANS):
    """Yield (label, case) for one family at one head_dim and PV type.

    scale_ladder, ramp: the families that depend on the loop shape.  scale_ladder spans every N of LOOP_NS x causal x
      granularity.  ramp spans the five steps of its PV type (thr = 6 or 3) x causal x granularity; the ascending staircase
      at every N of LOOP_NS, the descending and sawtooth ones at N = 456 (their point is the order of the maxima, not the
      ring slot a tile lands in).
    extreme_s, one_hot, coarse_lsb, big_v: properties of one tile's arithmetic, N = 456 only (six full tiles and a ragged
      one), x causal x granularity."""
    g0 = grans[0]
    for causal in (False, True):
        if family in ("scale_ladder", "coarse_lsb", "big_v"):  # the scales, hence the logits, depend on the granularity
            for gran in grans:
                tag = f"{'causal' if causal else 'full'}-{gran}"
                if family == "scale_ladder":
                    for N in LOOP_NS:
                        yield f"N{N}-{tag}", scale_ladder(D, N, causal, gran)
                elif family == "coarse_lsb":
                    for e in (-6, -5, -4):
                        yield f"lsb2^{e}-{tag}", coarse_lsb(D, N_ONE, causal, gran, e)
                else:
                    yield tag, big_v(D, N_ONE, causal, gran)
            continue
        base = []  # uniform scales: one set of logits, laid out for each granularity
        if family == "ramp":
            for step in ramp_steps(pv):
                for shape in RAMP_SHAPES:
                    for N in (LOOP_NS if shape == "ascending" else (N_ONE,)):
                        base.append((f"{shape}-step{step}-N{N}", ramp(D, N, causal, g0, step, shape)))
        elif family == "extreme_s":
            for variant in ("corner", "zero"):
                base.append((variant, extreme_s(D, N_ONE, causal, g0, variant)))
        elif family == "one_hot":
            for where in ONE_HOT_KEYS:
                base.append((where, one_hot(D, N_ONE, causal, g0, where)))
                base.append((f"{where}-subnormal", one_hot(D, N_ONE, causal, g0, where, subnormal=True)))
        else:
            raise ValueError(family)
        for label, c in base:
            for gran in grans:
                yield f"{label}-{'causal' if causal else 'full'}-{gran}", (c if gran == g0 else regran(c, gran))


def uniform_case(v, causal, M):
    """The case a degenerate operator call reduces to: all logits equal (S = 0), so every row weighs its keys uniformly.
    ``v`` is the fp16 or bf16 V [1,1,N,D] the operator was given; the e4m3 triple is the operator's own quantizer
    (oracle.per_channel_fp8 without smoothing, bit-exact against the HIP quantizer in tests/test_gpu_parity.py).  The
    output dtype follows ``v``."""
    N, D = v.shape[2], v.shape[3]
    v8t, vsc, _ = O.per_channel_fp8(v, "HND", smooth_v=False)
    return dict(q8=torch.zeros(B, HQ, M, D, dtype=torch.int8), k8=torch.zeros(B, HK, N, D, dtype=torch.int8),
                q_scale_rows=torch.ones(B, HQ, M), k_scale_cols=torch.ones(B, HK, N), logit_mult=1.0, causal=causal,
                M=M, N=N, D=D, family="degenerate", v_f16=v, v_bf16=v, v_f8t=v8t, v_scale=vsc, out_dtype=v.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# split-KV: the key ranges, the bound of the merged result, and a float64 restatement that can make one deliberate mistake
# ---------------------------------------------------------------------------------------------------------------------

U32 = 2.0 ** -24


def split_ranges(length, S):
    """[(t0, t1)] of the NON-EMPTY splits of ``length`` keys under S splits (include/sageattn_hip.h, split-KV attention):
    ntk = ceil(length / 64), tps = ceil(ntk / S), split s owns the tiles [s * tps, min((s + 1) * tps, ntk))"""
    ntk = O.cdiv(length, 64)
    tps = O.cdiv(ntk, S) if ntk else 0
    return [(s * tps, min((s + 1) * tps, ntk)) for s in range(S) if tps and s * tps < ntk]


def split_subcases(c, S, length=None):
    """the subcase of every non-empty split, in split order"""
    length = c["N"] if length is None else length
    return [cached_subcase(c, range(t0, t1), length) for t0, t1 in split_ranges(length, S)]


def _merge_eps(lmax):
    """seqpar_ref.merge_eps on base-2 LSEs: the device's exp / log allowance EPS_EXP plus the fp32 roundings of l_s - mx and
    of mx + log2(sum), each 2^-24 of at most max_s |l_s| (a rounding of the exponent by x moves the weight by 2^x - 1 <= x)"""
    from seqpar_ref import EPS_EXP
    return EPS_EXP + 3 * U32 * (1 + lmax)


def merged_bound(c, pv, splits, out_dtype=None):
    """Per-element tolerance of a split-KV result (the merged o in ``out_dtype`` and the merged RAW base-2 lse2) against
    reference64 of ``c`` (the full case, or its ``length`` subcase) -> (o_bound [1,Hq,M,D], lse2_bound [1,Hq,M]).

    With o_s, l_s the exact (fp64) partial results of the non-empty splits s, W_s = 2^(l_s - lse2) their exact weights
    (sum_s W_s = 1, sum_s W_s o_s = o64), B_s / L_s the ``bound`` of split s's subcase WITHOUT output ulps (the workspace is
    fp32; L_s keeps its two fp32 ulps, the partial LSE is stored in fp32) and x_s, k_s what the kernel stored:

      |o - o64| <= (1 + rho) * sum_s W_s B_s  +  (rho + eps) * sum_s W_s (|o_s| + B_s)  +  half an output ulp
      |lse2 - lse2_64| <= max_s L_s + log2(e) * eps + 2^-23 |lse2_64|

    * |x_s - o_s| <= B_s and |k_s - l_s| <= L_s: ``bound`` on the subcase, proved sound there.
    * rho = 2^(L_a + L_b) - 1, L_a and L_b the two largest L_s of the row (0 with one non-empty split, whose weight is 1):
      the kernel's normalised weight of split s is 2^(k_s) / sum_r 2^(k_r); numerator and denominator move by at most
      2^(+-L) each and two splits may err in opposite directions, so it lies within (1 +- rho) W_s.  First term: the
      partials' own errors under the moved weights; second: the moved weights on the partials themselves.
    * eps = seqpar_ref.EPS_EXP + 3 * 2^-24 * (1 + max_s |l_s|) + (S + 2) * 2^-24: the merge's own fp32 arithmetic -- the
      project's allowance for the device's exp / log pair (no new measured constant), the roundings of l_s - mx and of
      mx + log2(sum) as seqpar_ref.merge_eps counts them (in base-2 units), and one rounding per addition of the <= S terms of
      sum_s w_s x_s, of the reciprocal and of the product with it, each at most 2^-24 of sum_s w_s |x_s|.
    * half an output ulp: the ONE rounding to ``out_dtype``, taken at |o64| + (the rest of the bound): the result may lie a
      binade above the reference (splitkv_util.merged_reference), never above that sum.
    * LSE: log2 sum_s 2^(k_s) is 1-Lipschitz in the sup norm of k, hence max_s L_s; a relative error eps of the sum is
      log2(e) * eps in its logarithm; 2^-23 |lse2_64| is the rounding of mx + log2f(sum) and log2f's own ulp.
    The finished natural-log LSE (lse2 / log2(e) + (q.km) * sm_scale) gets ``finish_bound`` on top."""
    out_dtype = OUT_DTYPE[pv] if out_dtype is None else out_dtype
    key, cache = ("merged_bound", pv, splits, out_dtype), c.setdefault("_cache", {})
    if key not in cache:
        cache[key] = _merged_bound(c, pv, splits, out_dtype)
    return cache[key]


def _merged_bound(c, pv, splits, out_dtype):
    ref = reference64(c, pv)
    subs = split_subcases(c, splits)
    if len(subs) == 1:
        o_b, l_b = bound(subs[0], pv, out_ulps=0)
        rest = o_b
    else:
        refs = [reference64(s, pv) for s in subs]
        bnds = [bound(s, pv, out_ulps=0) for s in subs]
        l = torch.stack([r["lse2"] for r in refs])                       # [S,1,Hq,M]
        W = torch.exp2(l - ref["lse2"]).unsqueeze(-1)
        Bs = torch.stack([b[0] for b in bnds])
        Ls = torch.stack([b[1] for b in bnds])
        top = Ls.topk(2, dim=0).values
        rho = (torch.exp2(top[0] + top[1]) - 1).unsqueeze(-1)
        eps = (_merge_eps(l.abs().amax(0)) + (len(subs) + 2) * U32).unsqueeze(-1)
        wabs = (W * (torch.stack([r["o"] for r in refs]).abs() + Bs)).sum(0)
        rest = (1 + rho) * (W * Bs).sum(0) + (rho + eps) * wabs
        l_b = Ls.amax(0) + K_LOG2E * eps.squeeze(-1) + 2 * U32 * ref["lse2"].abs()
    o_b = rest + 0.5 * out_ulp(ref["o"].abs() + rest, pv, out_dtype)
    return o_b, l_b


def finish_lse64(lse2, qkm):
    """the natural-log LSE of the fused-Q entry points in float64: lse2 / log2(e) + (q . km) * sm_scale (``qkm`` holds the
    product)"""
    return lse2 / math.log2(math.e) + qkm


def finish_bound(l2_b, lse2_64, qkm):
    """bound of the FINISHED LSE given the bound of the raw lse2: ln 2 times it, plus the four fp32 roundings of the finish
    lse2 / log2(e) + (q.km) * sm_scale (the constant, the product, the quotient, the sum), each at most 2^-24 of the largest
    magnitude involved -- as test_operators_on_zero_q_rows_and_constant_k counts them"""
    nat = lse2_64 / math.log2(math.e)
    mag = torch.maximum(torch.maximum(nat.abs(), qkm.abs()), (nat + qkm).abs())
    return l2_b * math.log(2) + 4 * U32 * mag


def merged_ratios(c, pv, splits, o, lse, qkm, out_dtype=None):
    """largest |o - o64| / merged_bound and |lse - lse64| / finish_bound(merged_bound) over ALL elements; ``lse`` is the
    finished natural-log LSE, ``qkm`` the exact (q . km) * sm_scale [1,Hq,M]; non-finite -> inf"""
    ref = reference64(c, pv)
    o_b, l2_b = merged_bound(c, pv, splits, out_dtype)
    o, lse = o.double(), lse.double()
    if not (torch.isfinite(o).all() and torch.isfinite(lse).all()):
        return float("inf"), float("inf")
    l_b = finish_bound(l2_b, ref["lse2"], qkm)
    return float(((o - ref["o"]).abs() / o_b).max()), float(((lse - finish_lse64(ref["lse2"], qkm)).abs() / l_b).max())


SUBSET_MISTAKES = ("list_position_for_tile_index", "length_rounded_up_to_tile")
SPLIT_MISTAKES = ("split_scales_from_tile0", "split_tail_unmasked", "merge_equal_weights", "merge_base_e_weights",
                  "merge_drops_last_split", "correction_added_per_split", "length_rounded_up_to_tile")


def _pad_keys(d):
    """the subcase with the zero padding of its last tile admitted as keys: k8 = 0 (S = 0), V = 0, the last key's scale"""
    n = d["N"]
    pad = O.cdiv(n, 64) * 64 - n
    if pad == 0:
        return d
    e = dict(d)
    e["_cache"] = {}
    z = lambda t: torch.cat([t, torch.zeros(B, HK, pad, t.shape[-1], dtype=t.dtype)], dim=2)
    e["k8"], e["v_f16"], e["v_bf16"] = z(d["k8"]), z(d["v_f16"]), z(d["v_bf16"])
    e["k_scale_cols"] = torch.cat([d["k_scale_cols"], d["k_scale_cols"][:, :, -1:].expand(B, HK, pad)], dim=-1)
    e["N"] = n + pad
    return e


def restate_subset64(c, pv, tiles=None, length=None, mistake=None):
    """restate64 (float64, no rounding) of a kernel that walks the listed tiles of ``c`` up to ``length`` keys -- without a
    mistake it equals reference64 of subcase(c, tiles, length); ``mistake`` makes one of SUBSET_MISTAKES:
    list_position_for_tile_index (the j-th listed tile takes the K scales of tile j), length_rounded_up_to_tile (the keys up
    to the next multiple of 64 -- real keys of ``c``, not padding -- are admitted)."""
    if mistake == "length_rounded_up_to_tile" and length is not None:
        length = min(O.cdiv(length, 64) * 64, c["N"])
    d = subcase(c, tiles, length)
    if mistake == "list_position_for_tile_index":
        d["k_scale_cols"] = c["k_scale_cols"][:, :, :O.cdiv(d["N"], 64) * 64][:, :, :d["N"]].contiguous()
    return restate64(d, pv)


def restate_split64(c, pv, S, lengths=None, mistake=None, qkm=None):
    """Split-KV in float64 with no rounding: the tile range of every split by the rule of include/sageattn_hip.h, restate64
    on each range, the merge in base 2 in split order (mx = max_s l_s, w_s = 2^(l_s - mx), o = sum w_s o_s / sum w_s, lse2 =
    mx + log2 sum w_s).  Without a mistake it equals reference64 of subcase(c, length=...) to float64 accuracy; ``mistake``
    makes exactly one of SPLIT_MISTAKES.  ``lengths``: None (all keys), one length, or a list (-> a list of results).
    -> (o, lse2), or (o, lse2, lse) with ``qkm`` [1,Hq,M], the exact (q . km) * sm_scale: lse is the finished LSE."""
    if isinstance(lengths, (list, tuple)):
        return [restate_split64(c, pv, S, n, mistake, qkm) for n in lengths]
    true_len = c["N"] if lengths is None else min(int(lengths), c["N"])
    length = true_len
    if mistake == "length_rounded_up_to_tile":
        length = min(O.cdiv(length, 64) * 64, c["N"])
    parts = []
    ranges = split_ranges(length, S)
    for i, (t0, t1) in enumerate(ranges):
        d = subcase(c, range(t0, t1), length)
        if mistake == "split_scales_from_tile0":
            d["k_scale_cols"] = c["k_scale_cols"][:, :, :d["N"]].contiguous()
        if mistake == "split_tail_unmasked" and i == len(ranges) - 1:
            d = _pad_keys(d)
        parts.append(restate64(d, pv))
    if mistake == "merge_drops_last_split" and len(parts) > 1:
        parts = parts[:-1]
    o = torch.stack([p[0] for p in parts])
    l = torch.stack([p[1] for p in parts])
    mx = l.amax(0)
    if mistake == "merge_equal_weights":
        w = torch.ones_like(l)
    elif mistake == "merge_base_e_weights":
        w = torch.exp(l - mx)
    else:
        w = torch.exp2(l - mx)
    sm = w.sum(0)
    res = ((w.unsqueeze(-1) * o).sum(0) / sm.unsqueeze(-1), mx + torch.log2(sm))
    if qkm is None:
        return res
    times = len(ranges) if mistake == "correction_added_per_split" else 1
    return res + (res[1] / math.log2(math.e) + times * qkm,)


def merge_fp32(o_parts, l2_parts):
    """The merge kernel's arithmetic in numpy float32, in split order (sage_attn_splitkv.hip): for the CPU soundness test.
    o_parts [S,...,D] and l2_parts [S,...] fp32 tensors -> (o fp32, lse2 fp32)"""
    import numpy as np
    o, l = o_parts.numpy().astype(np.float32), l2_parts.numpy().astype(np.float32)
    mx = l.max(0)
    acc, sm = np.zeros_like(o[0]), np.zeros_like(mx)
    for s in range(l.shape[0]):
        w = np.exp2(l[s] - mx).astype(np.float32)
        sm = (sm + w).astype(np.float32)
        acc = (acc + o[s] * w[..., None]).astype(np.float32)
    inv = (np.float32(1) / sm).astype(np.float32)
    return torch.from_numpy(acc * inv[..., None]), torch.from_numpy((mx + np.log2(sm)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# the subset configurations (shared by the CPU soundness test and tests/test_constructed_subsets_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------

SUBSET_N = 456  # 7 whole tiles and a ragged one of 8 keys (tile 7); M = 150: two q-blocks
# name -> tile lists [head][q-block]
SUBSET_MAPS = {
    "alternate": [[[1, 3, 5, 7]] * 2] * 2,
    "ragged_only": [[[7]] * 2] * 2,
    "first_last": [[[0, 7]] * 2] * 2,
    "middle": [[[3]] * 2] * 2,
    "mixed": [[[0, 2, 4, 6], [1, 3, 5, 7]], [[2, 3], [0, 5, 7]]],  # differs between the q-blocks and between the heads
}
KVLEN_LENGTHS = (SUBSET_N, 257, 64, 1)
SPLIT_CONFIGS = ((512, (2, 3, 4, 5, 8, 9, 16)), (456, (2, 3, 7)))  # (N, the split counts run at it)
SPLIT_LENGTHS = (None, 257, 0)  # per batch: all keys, 257, none


def map_tensor(name, ntk=None):
    """bool [1, Hq, 2, ntk] of a SUBSET_MAPS entry"""
    ntk = O.cdiv(SUBSET_N, 64) if ntk is None else ntk
    bm = torch.zeros(1, HQ, 2, ntk, dtype=torch.bool)
    for h in range(HQ):
        for qb in range(2):
            bm[0, h, qb, SUBSET_MAPS[name][h][qb]] = True
    return bm


def subset_cases(family, D, pv, grans=("per_warp", "per_thread"), causal=False, N=SUBSET_N):
    """Yield (label, case) of the families run through a block map or a key length, at N = 456.
    scale_ladder per granularity; ramp ascending at the steps around the lazy threshold of the PV type and at 40, sawtooth at
    40; one_hot with the hot key at 0 (tile 0), 200 (tile 3), 257 (tile 4: the first key past the length 257) and 448 (the
    ragged tile): every map lists some of them and not the others; extreme_s corner and zero."""
    tag = "causal" if causal else "full"
    if family == "scale_ladder":
        for gran in grans:
            yield f"{tag}-{gran}", scale_ladder(D, N, causal, gran)
        return
    t = "6" if pv != "fp8" else "3"
    base = {
        "ramp": [(f"{shape}-step{st}", lambda st=st, shape=shape: ramp(D, N, causal, grans[0], st, shape))
                 for st, shape in ((t + "-", "ascending"), (t, "ascending"), (t + "+", "ascending"), ("40", "ascending"),
                                   ("40", "sawtooth"))],
        "one_hot": [(f"hot{k}", lambda k=k: one_hot(D, N, causal, grans[0], k)) for k in (0, 200, 257, 448)],
        "extreme_s": [(v, lambda v=v: extreme_s(D, N, causal, grans[0], v)) for v in ("corner", "zero")],
    }[family]
    for label, build in base:
        c = build()
        for gran in grans:
            yield f"{label}-{tag}-{gran}", (c if gran == grans[0] else regran(c, gran))


SUBSET_FAMILIES = ("scale_ladder", "ramp", "one_hot", "extreme_s")
SPLIT_FAMILIES = ("ramp", "offset", "scale_ladder", "one_hot", "extreme_s")


def split_cases(family, D, N, gran):
    """Yield (label, anchored case) of the families run through split-KV at N keys (non-causal, M = 150).
    ramp: step 40, ascending / descending / sawtooth and "peak" (levels 0 2 4 6 7 5 3 1) -- for the rows with r > 0 the dominant
    split is the last, the first, the last and a MIDDLE one (the sawtooth's maximum is its last tile); ascending at step
    0.5: weights within a factor of 2^14 of each other, where a merge in the wrong base shows; offset (N = 512 only);
    scale_ladder; one_hot with the hot key in the first, a middle and the last split whatever S (keys 0, 200, N - 1);
    extreme_s zero: uniform weights, the merged o is the mean over all keys."""
    if family == "ramp":
        for shape in RAMP_SHAPES + ("peak",):
            yield f"{shape}-step40", ramp(D, N, False, gran, "40", shape, anchor=True)
        yield "ascending-step0.5", ramp(D, N, False, gran, "0.5", "ascending", anchor=True)
    elif family == "offset":
        if N == 512:
            yield "offset", offset(D, N, gran)
    elif family == "scale_ladder":
        yield "ladder", anchor(scale_ladder(D, N, False, gran))
    elif family == "one_hot":
        for k in (0, 200, N - 1):
            yield f"hot{k}", anchor(one_hot(D, N, False, gran, k))
    elif family == "extreme_s":
        yield "zero", anchor(extreme_s(D, N, False, gran, "zero"))
    else:
        raise ValueError(family)


def split_km(D, nonzero):
    """km [1,1,D] fp32: zeros, or multiples of 1/8 in [-2, 2] (q . km is then exact in fp32 in any summation order: every
    product q8 * 2^e * km is a multiple of 2^(e-3) below 2^(e+8), the sum of 128 of them below 2^24 such units)"""
    if not nonzero:
        return torch.zeros(1, HK, D)
    g = torch.Generator().manual_seed(970 + D)
    return torch.randint(-16, 17, (1, HK, D), generator=g).float() / 8


def split_qkm(c, km):
    """the exact (q . km) * sm_scale [1,Hq,M] in float64, sm_scale at its fp32 value"""
    q = c["q8"].double() * c["q_scale_rows"].double().unsqueeze(-1)
    return (q * km.double().repeat_interleave(HQ // HK, dim=1).unsqueeze(2)).sum(-1) * float(c["sm_scale"])


def split_gaps(c, pv, S, length=None):
    """largest difference between the fp64 LSEs (base 2) of two non-empty splits, per row [1,Hq,M]"""
    l = torch.stack([reference64(d, pv)["lse2"] for d in split_subcases(c, S, length)])
    return l.amax(0) - l.amin(0)


# ---------------------------------------------------------------------------------------------------------------------
# attn_mask: structured masks as part of a case (the CPU soundness test and tests/test_constructed_masks_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------

MASK_BM = 2
MASK_SMALL_SHAPES = ((1, 1), (5, 3), (33, 65), (128, 64))  # N = 3: every run of four keys crosses N; 65: one key in tile 1
BOOL_PATTERNS = ("late_first_key", "wave_tile_skip", "single_key", "ragged_only", "key_padding", "first_tile_off", "row_switch")
ADD_PATTERNS = ("grid", "pad_1e4", "neg_inf", "rows_1e4", "row_const")
SMALL_PATTERNS = ("late_first_key", "neg_inf")  # one bool and one additive pattern defined at every (M, N)
KEY_PAD_LEN = 257


def with_mask(c, mask, name=None):
    """A copy of the case that carries ``mask`` [Bm,Hq,M,N] (bool, or fp16 / bf16 additive base-2 terms), with a fresh cache.
    ``name``: the copy's cache is kept in the cache of ``c`` under that name, so that the regran copies of ``c`` (same logits)
    share the masked reference as they share the plain one."""
    assert not c["causal"] and tuple(mask.shape[1:]) == (HQ, c["M"], c["N"]) and mask.shape[0] in (1, 2)
    assert mask.dtype in (torch.bool, torch.float16, torch.bfloat16)
    d = dict(c)
    d["mask"] = mask
    d["_cache"] = {} if name is None else c.setdefault("_cache", {}).setdefault(("mask", name, mask.dtype), {})
    return d


def cut_case(c, M, N, causal=None):
    """the case cut to its first M rows and N keys, compact scales included (both layouts are prefix-compatible).
    ``causal`` (default: as the parent): the copy is marked causal or not whatever the parent was -- the operands of a family do
    not depend on the flag, and ``allowed`` is the TOP-LEFT mask n <= m for any (M, N), under which every row keeps key 0.  A
    causal cut with more than 150 rows is taken from a causal parent (M = N).  N = 0: the keyless sequence of ``pack``, a case
    with queries only; it has no reference."""
    causal = c["causal"] if causal is None else bool(causal)
    assert 0 < M <= c["M"] and 0 <= N <= c["N"] and c.get("mask") is None
    if N > 0:
        d = subcase(c, length=N)
    else:
        d = {k: v for k, v in c.items() if k not in ("k_scale", "_cache")}
        d["_cache"] = {}
        for key in ("k8", "v_f16", "v_bf16"):
            d[key] = c[key][:, :, :0].contiguous()
        d["k_scale_cols"], d["v_f8t"], d["N"] = c["k_scale_cols"][..., :0].contiguous(), c["v_f8t"][..., :0].contiguous(), 0
    _, gq = _gid_q(M, c["gran"])
    gk = _gid_k(N, c["gran"])[1] if N else 0
    d.update(q8=c["q8"][:, :, :M].contiguous(), q_scale=c["q_scale"][..., :gq].contiguous(),
             q_scale_rows=c["q_scale_rows"][..., :M].contiguous(), k_scale=c["k_scale"][..., :gk].contiguous(), M=M,
             causal=causal)
    assert torch.equal(O.expand_q_scale(d["q_scale"], M, c["gran"]), d["q_scale_rows"])
    assert N == 0 or torch.equal(O.expand_k_scale(d["k_scale"], N, c["gran"]), d["k_scale_cols"])
    return d


def _mask_index(M, N, Bm):
    b, h = torch.arange(Bm).view(Bm, 1, 1, 1), torch.arange(HQ).view(1, HQ, 1, 1)
    return b, h, torch.arange(M).view(1, 1, M, 1), torch.arange(N).view(1, 1, 1, N), 3 * b + h


def lone_row_tile(s):
    """wave_tile_skip: the kept tile of wave 0 in which row 31 alone keeps keys, for the slice shift s = 3 b + h"""
    return 1 if (1 + s) % 3 else 2


def mask_pattern(name, M=M_FULL, N=SUBSET_N, dtype=torch.float16, Bm=MASK_BM):
    """One named mask [Bm,Hq,M,N]: bool for BOOL_PATTERNS, ``dtype`` (fp16 / bf16, every value exact in both) for ADD_PATTERNS.
    The broadcastable patterns (key_padding, row_switch, row_const) are EXPANDED VIEWS of their compact tensor (stride 0).
    s = 3 b + h is the shift of slice (b, h): it enters every bool pattern that depends on the key, so no two slices are equal
    (row_switch names rows only and is the same on every slice; key_padding is [Bm,1,1,N] and differs between the batches).

    late_first_key  row r's first key is (37 r + s) % N; beyond it the row keeps the keys with (n + r + s) % 3 != 0
    wave_tile_skip  the 32x64 tile (g, j) is off iff (g + j + s) % 3 == 0 (waves of one q-block skip different tiles, some
                    wave has tile 0 off); kept tiles hold the checkerboard (r + n + s) % 2 == 0; in tile lone_row_tile(s) of
                    wave 0 rows 0..30 are off and row 31 alone is on
    single_key      row r keeps key (61 r + s) % N only
    ragged_only     rows of odd waves keep the keys >= 64 * ((N - 1) // 64) + s only (N = 456: 448 + s .. 455); even waves all
    key_padding     keys >= 257 - 3 b off for every row, [Bm,1,1,N] expanded
    first_tile_off  keys below 64 + (r + s) % 5 off
    row_switch      [Bm,Hq,M,1] expanded over the keys: rows with r % 16 == 5 off entirely -- the only rows of any pattern
                    that keep no key -- the others fully on
    grid            multiples of 1/16 in [-8, 8]: ((7 r + 13 n + 29 h + 53 b) % 257 - 128) / 16
    pad_1e4         grid, keys >= 257 at -1e4 (in the mask dtype: bf16 holds -9984)
    neg_inf         grid, the keys with (n + r) % 3 == 0 and those below (64 + r % 5) % N at -inf; a row that would keep no key
                    (possible for N < 70 only) keeps key N - 1
    rows_1e4        grid, rows with r % 7 == 3 entirely at -1e4
    row_const       3 * ((r + s) % 11) - 15, [Bm,Hq,M,1] expanded"""
    b, h, r, n, s = _mask_index(M, N, Bm)
    full = (Bm, HQ, M, N)
    if name == "late_first_key":
        first = (37 * r + s) % N
        return ((n == first) | ((n > first) & ((n + r + s) % 3 != 0))).expand(full).contiguous()
    if name == "wave_tile_skip":
        g, j = r // 32, n // 64
        ok = ((g + j + s) % 3 != 0) & ((r + n + s) % 2 == 0)
        lone = torch.where((1 + s) % 3 != 0, 1, 2)
        ok = ok & ~((g == 0) & (j == lone) & (r < 31))
        return ok.expand(full).contiguous()
    if name == "single_key":
        return (n == (61 * r + s) % N).expand(full).contiguous()
    if name == "ragged_only":
        start = 64 * ((N - 1) // 64) + s
        assert int(start.max()) < N
        return (((r // 32) % 2 == 0) | (n >= start)).expand(full).contiguous()
    if name == "key_padding":
        assert N > KEY_PAD_LEN
        return (n < KEY_PAD_LEN - 3 * b).contiguous().expand(full)
    if name == "first_tile_off":
        assert N > 69
        return (n >= 64 + (r + s) % 5).expand(full).contiguous()
    if name == "row_switch":
        return (r % 16 != 5).expand(Bm, HQ, M, 1).contiguous().expand(full)
    assert name in ADD_PATTERNS, name
    assert dtype in (torch.float16, torch.bfloat16)
    if name == "row_const":
        m = (3 * ((r + s) % 11) - 15).to(dtype).expand(Bm, HQ, M, 1).contiguous()
        return m.expand(full)
    grid = (((7 * r + 13 * n + 29 * h + 53 * b) % 257 - 128).double() / 16).expand(full).clone()
    assert torch.equal(grid.to(dtype).double(), grid) and float(grid.abs().max()) <= 8.0
    if name == "pad_1e4":
        assert N > KEY_PAD_LEN
        grid[..., KEY_PAD_LEN:] = -1.0e4
    elif name == "neg_inf":
        off = (((n + r) % 3 == 0) | (n < (64 + r % 5) % N)).expand(full).clone()
        empty = off.all(-1)
        off[..., N - 1] &= ~empty
        grid = grid.masked_fill(off, float("-inf"))
    elif name == "rows_1e4":
        grid = torch.where((r % 7 == 3).expand(full), torch.full_like(grid, -1.0e4), grid)
    return grid.to(dtype)


def mask_patterns(M=M_FULL, N=SUBSET_N, dtype=torch.float16, Bm=MASK_BM, names=None):
    """yield (name, mask) of every pattern (``names``: of those) at M rows and N keys; M = 150, N = 456 is two q-blocks, five
    32-row waves of which the last holds 22 valid rows, seven whole tiles and a ragged one of 8 keys"""
    for name in (BOOL_PATTERNS + ADD_PATTERNS if names is None else names):
        yield name, mask_pattern(name, M, N, dtype, Bm)


def no_key_rows(c):
    """bool [Bm,Hq,M]: the rows that keep no key (row_switch only)"""
    return ~allowed(c).any(-1)


def mask_ratio_tensors(c, pv, o, lse2):
    """ratio_tensors of a masked case with reference and bound kept in the case's cache; the rows that keep no key hold 0
    (they are undefined: include/sageattn_hip.h) -> (ro [Bm,Hq,M,D], rl [Bm,Hq,M], rows without a key [Bm,Hq,M])"""
    cache = c.setdefault("_cache", {})
    if ("bound", pv) not in cache:
        cache[("bound", pv)] = bound(c, pv) + (no_key_rows(c),)
    o_b, l_b, dead = cache[("bound", pv)]
    ref = reference64(c, pv)
    inf = torch.tensor(float("inf"), dtype=torch.float64)
    o, lse2 = o.double(), lse2.double()
    ro = torch.where(torch.isfinite(o), (o - ref["o"]).abs() / o_b, inf)
    rl = torch.where(torch.isfinite(lse2), (lse2 - ref["lse2"]).abs() / l_b, inf)
    zero = torch.zeros((), dtype=torch.float64)
    return torch.where(dead.unsqueeze(-1), zero, ro), torch.where(dead, zero, rl), dead


def mask_ratios(c, pv, o, lse2):
    """largest ratio over every element of every row that keeps a key -> (o, lse2); NaN (a broken reference) -> inf"""
    ro, rl, _ = mask_ratio_tensors(c, pv, o, lse2)
    f = lambda x: float("inf") if bool(torch.isnan(x).any()) else float(x.max())
    return f(ro), f(rl)


MASK_MISTAKES = ("mask_next_row", "mask_next_key", "mask_head_zero", "mask_batch_zero", "skip_by_first_row", "tail_run_unread",
                 "run_reversed", "additive_times_scale", "additive_in_nats", "bf16_read_as_fp16")


def restate_mask64(c, pv, mistake=None):
    """restate64 (float64, no rounding) of the attn_mask loop on a case that carries a mask: the mask is read, applied to the
    logits, and the tile loop runs.  Without a mistake it equals reference64 to float64 accuracy; ``mistake`` makes exactly
    one of MASK_MISTAKES:
      mask_next_row / mask_next_key  row r reads the mask of row r + 1 / key n that of key n + 1 (the last one its own)
      mask_head_zero / mask_batch_zero  every head reads head 0's slice / every batch batch 0's
      skip_by_first_row   a 32-row wave skips a 64-key tile when its FIRST row keeps no key there
      tail_run_unread     the keys of the run of four that crosses N count as allowed (additive: term 0)
      run_reversed        the four mask values of every whole run of four keys in reverse order
      additive_times_scale  the additive term multiplied by the key's dequantisation scale
      additive_in_nats    the additive term taken as natural-log units (times log2 e)
      bf16_read_as_fp16   the 16 bits of a bf16 term read as fp16"""
    mask = c["mask"]
    M, N = c["M"], c["N"]
    is_bool = mask.dtype == torch.bool
    mk = mask.clone()
    if mistake == "mask_next_row":
        mk = mk[:, :, (torch.arange(M) + 1).clamp(max=M - 1)]
    elif mistake == "mask_next_key":
        mk = mk[..., (torch.arange(N) + 1).clamp(max=N - 1)]
    elif mistake == "mask_head_zero":
        mk = mk[:, :1].expand_as(mk).clone()
    elif mistake == "mask_batch_zero":
        mk = mk[:1].expand_as(mk).clone()
    elif mistake == "tail_run_unread":
        mk[..., 4 * (N // 4):] = True if is_bool else 0.0
    elif mistake == "run_reversed":
        n = torch.arange(4 * (N // 4))
        mk[..., :n.numel()] = mk[..., 4 * (n // 4) + 3 - n % 4]
    elif mistake == "bf16_read_as_fp16":
        assert mask.dtype == torch.bfloat16
        mk = mk.view(torch.int16).view(torch.float16)
    ok = mk if is_bool else mk.float() > float("-inf")
    if mistake == "skip_by_first_row":
        ok = ok.clone()
        for r0 in range(0, M, 32):
            for n0 in range(0, N, 64):
                dead = ~ok[:, :, r0, n0:n0 + 64].any(-1)
                ok[:, :, r0:r0 + 32, n0:n0 + 64] &= ~dead.view(*dead.shape, 1, 1)
    t = scores(c) * scale_matrix(c)
    if not is_bool:
        add = torch.where(torch.isinf(mk.double()), torch.zeros((), dtype=torch.float64), mk.double())  # -inf lives in ``ok``
        if mistake == "additive_times_scale":
            add = add * scale_matrix(c)
        elif mistake == "additive_in_nats":
            add = add * math.log2(math.e)
        t = t + add
    t = t.expand(ok.shape).masked_fill(~ok, float("-inf"))
    return _lazy_loop64(t, v64(c, pv), pv)


PUBLIC_BACKENDS = {"triton": "per_thread", "cuda": "per_block"}  # quantization_backend -> the granularity it quantizes with
PUBLIC_PATTERNS = ("key_padding", "late_first_key", "neg_inf")


def public_form(c, backend):
    """The case in the form sageattn_qk_int8_pv_fp16_triton(q, k, v, attn_mask=..., smooth_k=False) reproduces from REAL
    q and k: BOTH quantizers must return the case's int8 operands and scales.  Two head-dim channels are reserved: D - 1 holds
    q8 = 127 / k8 = 0 (``anchor``) and D - 2 holds k8 = 127 / q8 = 0, so every quantization group of Q and of K has amax
    127 * 2^e and neither channel adds to a score.  The smallest q and k scale are moved to 2^1 (the per-thread numerics add
    1e-7 to a scale, which fp32 absorbs from 2^1 up) and logit_mult takes the rest, as a power of two again:
      "triton"  per-thread scales; ``sm_scale`` with fp32(sm_scale) * kLog2e = 2^x exactly (the kernel forms that product)
      "cuda"    per-block scales with sm_scale * 1.44269504 folded into Q by the quantizer: ``sm_scale`` = 2^x / 1.44269504 in
                double precision, whose product with the constant rounds to 2^x in fp32; the case's q_scale is the FOLDED scale
                the quantizer returns and its logit_mult is 1 (the kernel is told logit_mult_is_one)
    ``q_real_rows`` / ``k_scale_cols``: what Q = q8 * 2^e and K = k8 * 2^e are formed with (``public_qk``).  K smoothing would
    subtract the key mean and lose the integers: the call must pass smooth_k=False."""
    gran = PUBLIC_BACKENDS[backend]
    assert c["gran"] == gran and not c["causal"] and not c.get("anchored")
    d = dict(c)
    d["q8"], d["k8"] = c["q8"].clone(), c["k8"].clone()
    d["q8"][..., -1], d["k8"][..., -1] = 127, 0
    d["q8"][..., -2], d["k8"][..., -2] = 0, 127
    fq = 2.0 ** (1 - int(torch.log2(c["q_scale"].min())))
    fk = 2.0 ** (1 - int(torch.log2(c["k_scale"].min())))
    for key, f in (("q_scale", fq), ("q_scale_rows", fq), ("k_scale", fk), ("k_scale_cols", fk)):
        d[key] = c[key] * f
    x = int(round(math.log2(c["logit_mult"] / (fq * fk))))
    d["q_real_rows"] = d["q_scale_rows"]
    if backend == "triton":
        d["sm_scale"], d["logit_mult"] = _pow2_logit_mult(x)
    else:
        d["sm_scale"], d["logit_mult"] = 2.0 ** x / 1.44269504, 1.0
        assert float(np.float32(d["sm_scale"] * 1.44269504)) == 2.0 ** x
        d["q_scale"], d["q_scale_rows"] = d["q_scale"] * 2.0 ** x, d["q_scale_rows"] * 2.0 ** x
    d["public"], d["_cache"] = backend, {}
    assert torch.equal(scale_matrix(d), scale_matrix(c))  # every logit scale is what it was
    return d


def public_qk(d, dtype):
    """Q = q8 * 2^e and K = k8 * 2^e of a ``public_form`` case in fp16 / bf16, exact -> (q [1,Hq,M,D], k [1,Hk,N,D])"""
    q = d["q8"].float() * d["q_real_rows"].unsqueeze(-1)
    k = d["k8"].float() * d["k_scale_cols"].unsqueeze(-1)
    assert torch.equal(q.to(dtype).float(), q) and torch.equal(k.to(dtype).float(), k)
    return q.to(dtype), k.to(dtype)


def public_cases(D, backend):
    """Yield (label, public_form case) run through the public entry: scale_ladder, one_hot (hot key 200), extreme_s zero"""
    gran = PUBLIC_BACKENDS[backend]
    yield "ladder", public_form(scale_ladder(D, SUBSET_N, False, gran), backend)
    yield "hot200", public_form(one_hot(D, SUBSET_N, False, gran, 200), backend)
    yield "zero", public_form(extreme_s(D, SUBSET_N, False, gran, "zero"), backend)


# ---------------------------------------------------------------------------------------------------------------------
# layouts: several cases in ONE call -- stacked over batches and KV heads, packed sequences, tile-major K / V (the CPU
# soundness test and tests/test_constructed_layouts_gpu.py).  Reference and bound stay those of each case: a slice of the
# call's result is held to the case that was put there.
# ---------------------------------------------------------------------------------------------------------------------

STACK_SHIFTS = ((0, 1), (2, 3))  # slot (b, hk): the power of two moved from its K scales into its Q scales


def rebalance(c, e):
    """The case with 2^e (e >= 0) moved from k_scale into q_scale: every product, hence every logit, reference and bound, is what
    it was (the copy shares the cache), while the scale TENSORS differ from the original's by a power of two -- so the slots of
    a stack carry K- and Q-scale ladders no two of which are equal, uniform families included."""
    assert e >= 0
    d, f = dict(c), 2.0 ** e
    for key, g in (("q_scale", f), ("q_scale_rows", f), ("k_scale", 1 / f), ("k_scale_cols", 1 / f)):
        d[key] = c[key] * g
    assert torch.equal(scale_matrix(d), scale_matrix(c))
    return d


def distinct_heads(c):
    """A rank-one family (ramp, one_hot) builds both query heads from one q8; the copy negates head 1 (the anchor channel of an
    anchored case apart), so that every row trend / the hot key's lead changes sign there and the two heads of the slot have
    different results: reading the other head's rows, scales or workspace slots then shows in every slot of a stack.  Another
    set of operands, hence a fresh cache; reference and bound come from the operands as always."""
    assert c["family"] in ("ramp", "one_hot") and int(c["q8"].abs().max()) <= 127 and torch.equal(c["q8"][:, 0], c["q8"][:, 1])
    d = dict(c)
    d["_cache"] = {}
    q8, Dd = c["q8"].clone(), c["D"] - (1 if c.get("anchored") else 0)
    q8[:, 1, :, :Dd] = -q8[:, 1, :, :Dd]
    d["q8"] = q8
    return d


def stack(cases):
    """One call's operands from a Bs x Hks grid of cases with equal (M, N, D, gran, causal): q8 [Bs, 2 Hks, M, D] (slot (b, hk)
    holds the query heads 2 hk, 2 hk + 1: GQA group 2), k8 [Bs, Hks, N, D], the compact scales [Bs, 2 Hks, Gq] / [Bs, Hks, Gk]
    and their expansions, the three V forms and v_scale [Bs, Hks, D].  ``grid`` keeps the cases: slice (b, hk) of a result is
    held to reference and bound of grid[b][hk], whose caches stay shared."""
    Bs, Hks = len(cases), len(cases[0])
    first = cases[0][0]
    same = ("M", "N", "D", "gran", "causal", "logit_mult", "sm_scale")
    assert all(len(row) == Hks and all(c[k] == first[k] for k in same) and c.get("mask") is None for row in cases for c in row)
    st = {k: first[k] for k in same}
    for key in ("q8", "k8", "q_scale", "k_scale", "q_scale_rows", "k_scale_cols", "v_f16", "v_bf16", "v_f8t", "v_scale"):
        st[key] = torch.cat([torch.cat([c[key] for c in row], dim=1) for row in cases], dim=0).contiguous()
    st.update(grid=[list(row) for row in cases], Bs=Bs, Hks=Hks, Hq=HQ * Hks, Hk=HK * Hks,
              anchored=all(c.get("anchored", False) for row in cases for c in row))
    return st


def stack_slots(D, N, causal, gran, anchored=False):
    """The standard 2 x 2 grid: (0, 0) scale_ladder, (0, 1) ramp ascending (step 40), (1, 0) one_hot with the LAST key hot,
    (1, 1) ramp descending (step 40), slot (b, hk) rebalanced by 2^STACK_SHIFTS[b][hk] -- the K scales of any two slots differ
    in at least three groups of four (asserted), by a power of two, and the two query heads of every slot differ
    (``distinct_heads``).  ``anchored``: the
    anchored forms, for the entry points that quantize Q themselves."""
    if anchored:
        raw = [[anchor(scale_ladder(D, N, causal, gran)), ramp(D, N, causal, gran, "40", "ascending", anchor=True)],
               [anchor(one_hot(D, N, causal, gran, "last")), ramp(D, N, causal, gran, "40", "descending", anchor=True)]]
    else:
        raw = [[scale_ladder(D, N, causal, gran), ramp(D, N, causal, gran, "40", "ascending")],
               [one_hot(D, N, causal, gran, "last"), ramp(D, N, causal, gran, "40", "descending")]]
    raw = [[c if c["family"] == "scale_ladder" else distinct_heads(c) for c in row] for row in raw]
    st = stack([[rebalance(c, STACK_SHIFTS[b][hk]) for hk, c in enumerate(row)] for b, row in enumerate(raw)])
    ks = st["k_scale"].reshape(4, -1)
    assert all(float((ks[i] != ks[j]).float().mean()) >= 0.75 for i in range(4) for j in range(i))  # (a ladder meets a uniform
    return st                                                                                         #  scale in 1 group of 7)


def stack_of(c):
    """a single case as a 1 x 1 stack"""
    return stack([[c]])


def slot_heads(hk):
    return slice(HQ * hk, HQ * hk + HQ)


def read_stack(st, b, hk, mistake=None):
    """Slot (b, hk) of a stacked call AS A KERNEL READS IT, again a case: query heads 2 hk, 2 hk + 1 of batch b, K / V / v_scale
    of (b, hk), the K scales of (b, hk).  Without a mistake these are the operands of grid[b][hk] bit for bit.
      head_scales_of_kv_head_0    the K scales of (b, 0)
      batch_operands_of_batch_0   K, V and v_scale of (0, hk); the scales (and any length) stay those of b"""
    own = st["grid"][b][hk]
    kb = 0 if mistake == "batch_operands_of_batch_0" else b
    sh = 0 if mistake == "head_scales_of_kv_head_0" else hk
    d = dict(own)
    d["_cache"] = {}
    for key in ("q8", "q_scale", "q_scale_rows"):
        d[key] = st[key][b:b + 1, slot_heads(hk)]
    for key in ("k8", "v_f16", "v_bf16", "v_f8t", "v_scale"):
        d[key] = st[key][kb:kb + 1, hk:hk + 1]
    for key in ("k_scale", "k_scale_cols"):
        d[key] = st[key][b:b + 1, sh:sh + 1]
    return d


def stack_ratios(st, pv, o, lse2, sub=None):
    """largest ``ratios`` over the slots of a stacked result o [Bs,Hq,M,D] / lse2 [Bs,Hq,M]; ``sub(case, b, hk)`` names the case
    a slot is held to (default: the slot's own)"""
    worst = (0.0, 0.0)
    for b in range(st["Bs"]):
        for hk in range(st["Hks"]):
            c = st["grid"][b][hk] if sub is None else sub(st["grid"][b][hk], b, hk)
            r = ratios(c, pv, o[b:b + 1, slot_heads(hk)], lse2[b:b + 1, slot_heads(hk)])
            worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    return worst


def interleaved_batch(st, b, h, mistake=None):
    """The batch whose key length the workgroup of (b, h) reads.  The kvlen / split-KV kernels number their workgroups with the
    batches alternating inside a head, id = h * B + b, and decode b = id % B.  ``interleave_b_h_swapped``: the length is taken
    with the id decoded batch-major, b' = id // Hq, while every operand address keeps (b, h)."""
    return (h * st["Bs"] + b) // st["Hq"] if mistake == "interleave_b_h_swapped" else b


def restate_stack64(st, pv, b, hk, mistake=None, lens=None):
    """restate64 (float64, no rounding) of slot (b, hk) of a stacked call, dense (``lens`` None) or with per-batch key lengths
    -> (o [1,2,M,D], lse2 [1,2,M]).  ``mistake``: one of read_stack's, or interleave_b_h_swapped."""
    d = read_stack(st, b, hk, mistake)
    if lens is None:
        return restate64(d, pv)
    parts = []
    for hl in range(HQ):
        n = lens[interleaved_batch(st, b, HQ * hk + hl, mistake)]
        o, l = restate64(subcase(d, length=n), pv)
        parts.append((o[:, hl:hl + 1], l[:, hl:hl + 1]))
    return torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=1)


def stack_km(st):
    """km [Bs,Hks,D] for the split-KV calls on a stack: split_km rolled by the slot number, so no two slots share it"""
    km = split_km(st["D"], True)
    return torch.cat([torch.cat([km.roll(2 * b + hk + 1, -1) for hk in range(st["Hks"])], dim=1) for b in range(st["Bs"])], dim=0)


def restate_stack_split64(st, pv, S, b, hk, length, qkm, mistake=None):
    """restate_split64 of slot (b, hk) of a stacked split-KV call -> (o, lse2, finished lse).  ``workspace_slot_of_head_0``: the
    merge of every head reads the partials in the workspace slots of head 0 of its batch (the finish keeps the row's own
    correction ``qkm``)."""
    if mistake != "workspace_slot_of_head_0":
        return restate_split64(read_stack(st, b, hk, mistake), pv, S, length, None, qkm)
    o, l2 = restate_split64(read_stack(st, b, 0), pv, S, length)
    o, l2 = o[:, :1].expand(-1, HQ, -1, -1), l2[:, :1].expand(-1, HQ, -1)
    return o, l2, l2 / math.log2(math.e) + qkm


# ---- packed sequences ----------------------------------------------------------------------------------------------------

PACK_CUTS = ((150, 456), (64, 65), (1, 1), (129, 320), (33, 0))  # (M_s, N_s); the last sequence has no key
PACK_CUTS_CAUSAL = ((150, 456), (65, 65), (200, 130))           # M_s < N_s, =, >


def pack(rows):
    """Packed-sequence operands (include/sageattn_hip.h, packed variable-length sequences).  ``rows[s]`` is the list of the Hks
    cut cases (one per KV head, or a single case) of sequence s, all of equal (M_s, N_s); every case of the pack has the same
    (D, gran, causal).  -> q8 [sum M_s, 2 Hks, D], k8 / v_f16 / v_bf16 [sum N_s, Hks, D], cu_q / cu_k int32 [S + 1], and the
    scales in the private layout q_scale [S, 2 Hks, Gq(max M_s)] / k_scale [S, Hks, Gk(max N_s)]: sequence s fills the first
    Gq(M_s) / Gk(N_s) slots of its rows, every other slot is NaN.  ``cases`` keeps the rows: heads 2 hk, 2 hk + 1 of sequence s
    are held to cases[s][hk]."""
    rows = [list(r) if isinstance(r, (list, tuple)) else [r] for r in rows]
    first, Hks = rows[0][0], len(rows[0])
    same = ("D", "gran", "causal", "logit_mult", "sm_scale")
    assert all(len(r) == Hks and all(c[k] == first[k] for k in same) and (c["M"], c["N"]) == (r[0]["M"], r[0]["N"])
               for r in rows for c in r)
    Ms, Ns = [r[0]["M"] for r in rows], [r[0]["N"] for r in rows]
    gran = first["gran"]
    gq, gk = _gid_q(max(Ms), gran)[1], _gid_k(max(Ns), gran)[1]
    pk = {k: first[k] for k in same}
    pk["q_scale"] = torch.full((len(rows), HQ * Hks, gq), float("nan"))
    pk["k_scale"] = torch.full((len(rows), HK * Hks, gk), float("nan"))
    for s, r in enumerate(rows):
        for hk, c in enumerate(r):
            pk["q_scale"][s, slot_heads(hk), :c["q_scale"].shape[-1]] = c["q_scale"][0]
            pk["k_scale"][s, hk, :c["k_scale"].shape[-1]] = c["k_scale"][0, 0]
    for key in ("q8", "k8", "v_f16", "v_bf16"):
        pk[key] = torch.cat([torch.cat([c[key][0] for c in r], dim=0).transpose(0, 1) for r in rows], dim=0).contiguous()
    cu = lambda lens: torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    pk.update(cases=rows, S=len(rows), Hks=Hks, Hq=HQ * Hks, Hk=HK * Hks, Ms=Ms, Ns=Ns, cu_q=cu(Ms), cu_k=cu(Ns), max_q=max(Ms),
              max_k=max(Ns), gq=gq, gk=gk)
    return pk


def pack_cases(D, gran, causal):
    """The sequences of the packed call, two KV heads (four query heads); KV head 1 holds the families of KV head 0 rotated by
    one sequence.  Non-causal, PACK_CUTS, KV head 0: scale_ladder (150, 456), ramp ascending (64, 65), one_hot with its hot
    key first (1, 1), ramp descending (129, 320), scale_ladder (33, 0).  Causal, PACK_CUTS_CAUSAL, cut from causal parents
    (M = N = 456): scale_ladder (150, 456), one_hot hot key 40 (65, 65), ramp sawtooth (200, 130).  The rank-one families with
    ``distinct_heads``; the case at (s, hk) rebalanced by 2^(s + 5 hk): no two alike."""
    if causal:
        par = [scale_ladder(D, 456, True, gran), one_hot(D, 456, True, gran, 40), ramp(D, 456, True, gran, "40", "sawtooth")]
        cuts = PACK_CUTS_CAUSAL
    else:
        par = [scale_ladder(D, 456, False, gran), ramp(D, 456, False, gran, "40", "ascending"),
               one_hot(D, 456, False, gran, "first"), ramp(D, 456, False, gran, "40", "descending"),
               scale_ladder(D, 456, False, gran)]
        cuts = PACK_CUTS
    par = [c if c["family"] == "scale_ladder" else distinct_heads(c) for c in par]
    n = len(par)
    return pack([[cut_case(rebalance(par[(s + hk) % n], s + 5 * hk), m, k, causal) for hk in range(2)]
                 for s, (m, k) in enumerate(cuts)])


def read_pack(pk, s, hk=0, mistake=None):
    """Heads 2 hk, 2 hk + 1 of sequence s of a packed call AS A KERNEL READS THEM, again a case: rows [cu_q[s], cu_q[s + 1]) of
    q8, rows [cu_k[s], cu_k[s + 1]) of k8 / v, the scale rows (s, h) of [S, H, G(max)] of which the first G(M_s) / G(N_s) slots
    count.
      cu_off_by_one_row             the K and V rows start at cu_k[s] + 1
      scales_of_previous_sequence   the K scale rows of sequence s - 1 (sequence 0: its own; the Q scales stay the sequence's:
                                    moved TOGETHER, the scales of two uniform families keep their product)
      scale_row_by_max_seqlen_of_q  the K scale row of (s, hk) at (s * Hk + hk) * Gq(max M_s) of the flat tensor"""
    own = pk["cases"][s][hk]
    M, N, gran = own["M"], own["N"], own["gran"]
    assert N > 0, "a sequence without keys has no softmax"
    q_lo, k_lo = int(pk["cu_q"][s]), int(pk["cu_k"][s]) + (1 if mistake == "cu_off_by_one_row" else 0)
    assert M == int(pk["cu_q"][s + 1]) - q_lo and N == int(pk["cu_k"][s + 1]) - int(pk["cu_k"][s])
    rows = (k_lo + torch.arange(N)).clamp(max=pk["k8"].shape[0] - 1)
    ss = max(s - 1, 0) if mistake == "scales_of_previous_sequence" else s
    gq_s, gk_s = _gid_q(M, gran)[1], _gid_k(N, gran)[1]
    d = dict(own)
    d["_cache"] = {}
    d["q8"] = pk["q8"][q_lo:q_lo + M, slot_heads(hk)].transpose(0, 1).unsqueeze(0)
    for key in ("k8", "v_f16", "v_bf16"):
        d[key] = pk[key][rows, hk:hk + 1].transpose(0, 1).unsqueeze(0)
    d["q_scale"] = pk["q_scale"][s:s + 1, slot_heads(hk), :gq_s]
    flat = pk["k_scale"].reshape(-1)
    row = pk["gq"] if mistake == "scale_row_by_max_seqlen_of_q" else pk["gk"]
    d["k_scale"] = flat[((ss * pk["Hk"] + hk) * row + torch.arange(gk_s)) % flat.numel()].view(1, 1, gk_s)
    d["q_scale_rows"], d["k_scale_cols"] = O.expand_q_scale(d["q_scale"], M, gran), O.expand_k_scale(d["k_scale"], N, gran)
    return d


def restate_pack64(pk, pv, s, hk=0, mistake=None):
    """restate64 of heads 2 hk, 2 hk + 1 of sequence s of a packed call; ``causal_bottom_right``: row m keeps the keys n <= m + (N_s - M_s) where the
    entry point's mask is top-left, n <= m (a row left without a key is NaN)"""
    d = read_pack(pk, s, hk, None if mistake == "causal_bottom_right" else mistake)
    return restate_causal64(d, pv, mistake) if mistake == "causal_bottom_right" else restate64(d, pv)


def restate_causal64(c, pv, mistake=None):
    """restate64 of a causal case of any (M, N); ``causal_bottom_right`` aligns the diagonal to the LAST key"""
    assert c["causal"]
    M, N = c["M"], c["N"]
    off = N - M if mistake == "causal_bottom_right" else 0
    ok = torch.arange(N).view(1, 1, 1, N) <= torch.arange(M).view(1, 1, M, 1) + off
    t = (scores(c) * scale_matrix(c)).masked_fill(~ok, float("-inf"))
    return _lazy_loop64(t, v64(c, pv), pv)


CAUSAL_CUTS = ((150, 456), (456, 150), (130, 129))  # top-left causal with M != N through the dense and kvlen kernels


def causal_cut_cases(D, gran):
    """(label, case) of CAUSAL_CUTS: scale_ladder at every shape, the sawtooth ramp (step 40) at (456, 150), all cut from
    causal parents"""
    lad, saw = scale_ladder(D, 456, True, gran), ramp(D, 456, True, gran, "40", "sawtooth")
    for m, n in CAUSAL_CUTS:
        yield f"ladder-{m}x{n}", cut_case(lad, m, n, True)
    yield "sawtooth-456x150", cut_case(saw, 456, 150, True)


# ---- tile-major K / V ----------------------------------------------------------------------------------------------------

TILE_GAP_ROWS = 8     # poisoned rows behind the 64 rows of every K / V tile
TILE_GAP_COLS = 16    # poisoned bytes behind the 64 tokens of every channel row of an e4m3 V^T tile
TILE_SCALE_SLOT = 8   # floats per (tile, b, hk) in the K-scale buffer: 4 | 1 scales, the rest NaN


def tile_major(c_or_stack):
    """K, V and the K scales of a case or a stack in the TILE-MAJOR layout of the sequence-parallel exchange buffers
    (include/sageattn_hip.h): k8 [T][B][Hk][64 + 8][D] int8, v_f16 / v_bf16 the same shape, v_f8t [T][B][Hk][D][64 + 16] e4m3
    (tokens in natural order), k_scale [T][B][Hk][8] -- the first 64 rows / 64 bytes / 4 | 1 floats of every block are the
    tile, the rest is poison (int8 127, NaN, 0x7F, NaN), and so are the K and fp16 / bf16 V rows behind key N - 1 in the ragged
    last tile.  (The e4m3 V^T keeps its ZEROS in [N, 64 T): the contract of the dense operand, whose last block the kernel
    reads whole.)  Tile strides are therefore larger than B * Hk tiles, and the K-scale strides are all non-zero.
    ``kt`` / ``vt`` / ``v8t`` / ``kst``: (stride_b, stride_h, stride_n | None, tile stride) in elements; ``layout(pv)``: the
    five sage_kv_layout values."""
    st = c_or_stack if "grid" in c_or_stack else stack_of(c_or_stack)
    Bs, Hk, N, D = st["Bs"], st["Hk"], st["N"], st["D"]
    T, R, W, SL = O.cdiv(N, 64), 64 + TILE_GAP_ROWS, 64 + TILE_GAP_COLS, TILE_SCALE_SLOT
    pt = 4 if st["gran"] == "per_thread" else 1
    tm = dict(st=st, T=T, per_tile=pt)
    tm["k8"] = torch.full((T, Bs, Hk, R, D), 127, dtype=torch.int8)
    tm["v_f16"] = torch.full((T, Bs, Hk, R, D), float("nan"), dtype=torch.float16)
    tm["v_bf16"] = torch.full((T, Bs, Hk, R, D), float("nan"), dtype=torch.bfloat16)
    v8 = torch.full((T, Bs, Hk, D, W), 0x7F, dtype=torch.uint8)
    tm["k_scale"] = torch.full((T, Bs, Hk, SL), float("nan"))
    for j in range(T):
        n = min(64, N - 64 * j)
        for key in ("k8", "v_f16", "v_bf16"):
            tm[key][j, :, :, :n] = st[key][:, :, 64 * j:64 * j + n]
        v8[j, :, :, :, :64] = st["v_f8t"].view(torch.uint8)[..., 64 * j:64 * j + 64]
        tm["k_scale"][j, :, :, :pt] = st["k_scale"][:, :, pt * j:pt * j + pt]
    tm["v_f8t"] = v8.view(torch.float8_e4m3fn)
    tm["kt"] = tm["vt"] = (Hk * R * D, R * D, D, Bs * Hk * R * D)
    tm["v8t"] = (Hk * D * W, D * W, W, Bs * Hk * D * W)
    tm["kst"] = (Hk * SL, SL, None, Bs * Hk * SL)
    tm["layout"] = lambda pv: (tm["kt"][3], tm["v8t"][3] if pv == "fp8" else tm["vt"][3], tm["kst"][0], tm["kst"][1], tm["kst"][3])
    return tm


def read_tiles(tm, b, hk, mistake=None):
    """Slot (b, hk) of a tile-major call AS A KERNEL READS IT, again a case: key r of (b, hk) is row r % 64 of tile r // 64, its
    scales the first 4 | 1 floats of that tile's slot.  K and the K scales are gathered from the FLAT buffers by their
    strides, V from its blocks.
      tile_stride_dense        tile j of K at 64 * stride_n * j behind tile 0 of (b, hk): the gap rows, then foreign tiles
      tile_scales_dense_layout the K scales at (b * Hk + hk) * T * (4 | 1) + (4 | 1) * j, the dense [B,Hk,Gk] strides"""
    st, T, pt = tm["st"], tm["T"], tm["per_tile"]
    own = st["grid"][b][hk]
    N, D, gran = st["N"], st["D"], st["gran"]
    r = torch.arange(N)
    sb, sh, sn, stile = tm["kt"]
    tile_of = 64 * sn if mistake == "tile_stride_dense" else stile
    flat_k = tm["k8"].reshape(-1, D)
    krow = ((b * sb + hk * sh + (r // 64) * tile_of + (r % 64) * sn) // D) % flat_k.shape[0]
    ksb, ksh, _, kst = tm["kst"]
    g = torch.arange(T * pt)
    if mistake == "tile_scales_dense_layout":
        kidx = (b * st["Hk"] + hk) * T * pt + g
    else:
        kidx = b * ksb + hk * ksh + (g // pt) * kst + g % pt
    d = dict(own)
    d["_cache"] = {}
    d["k8"] = flat_k[krow].view(1, 1, N, D)
    d["k_scale"] = tm["k_scale"].reshape(-1)[kidx % tm["k_scale"].numel()].view(1, 1, -1)
    d["k_scale_cols"] = O.expand_k_scale(d["k_scale"], N, gran)
    for key in ("v_f16", "v_bf16"):
        d[key] = tm[key][:, b, hk, :64].reshape(1, 1, T * 64, D)[:, :, :N]
    d["v_f8t"] = tm["v_f8t"].view(torch.uint8)[:, b, hk, :, :64].permute(1, 0, 2).reshape(1, 1, D, T * 64).view(torch.float8_e4m3fn)
    return d


LAYOUT_MISTAKES = ("head_scales_of_kv_head_0", "batch_operands_of_batch_0", "interleave_b_h_swapped", "workspace_slot_of_head_0",
                   "cu_off_by_one_row", "scales_of_previous_sequence", "scale_row_by_max_seqlen_of_q", "causal_bottom_right",
                   "tile_scales_dense_layout", "tile_stride_dense")
STACK_KV_LENS = ((257, 456), (456, 64))
