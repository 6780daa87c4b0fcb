"""sageattn_varlen in every geometry it can dispatch to: 4-wave (128-row q-blocks) and 8-wave (256-row q-blocks) workgroups
with cu_seqlens, causal with different q and k lengths per sequence (top-left mask), every split of a sequence's tiles into
fast-loop tiles, tail tiles and a ragged or aligned last tile inside one launch, ``max_seqlen_*`` given as upper bounds,
isolation between neighbouring sequences, ``sm_scale`` / ``smooth_k=False`` and a keyless sequence under a causal mask.

References: ``oracle.sage_oracle.sageattn_varlen_oracle`` (memoised per input: geometry variants share one result) with the
suite's bounds -- fp16 ``|o - oo| <= 4 * 2**-10 * max(|oo|, 0.25)``, bf16 ``max |o - oo| < 1.6e-2`` -- and exact float64
attention per sequence at 0.08 absolute.  Every test prints its largest deviation before it asserts."""
import functools

import numpy as np
import pytest
import torch

HQ, HK = 4, 2  # GQA
F16, BF16 = torch.float16, torch.bfloat16

LADDER = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 384, 449]
LENGTHS = {
    "ladder": (LADDER, LADDER),
    "cross": ([300, 5, 130, 64, 257, 1], [130, 300, 64, 257, 1, 200]),
    "long": ([70, 300, 129], [3136, 65, 200]),
    "isolation": ([70, 50, 130], [70, 50, 130]),
    "nokeys": ([70, 200, 33], [128, 0, 40]),
}
SEEDS = {"ladder": 1100, "cross": 1200, "long": 1300, "isolation": 1400, "nokeys": 1500}


def _cu(lens, dtype=torch.int32):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=dtype)


@functools.lru_cache(maxsize=None)
def _inputs(name, D, dt):
    """(q, k, v) of a case, seeded on the CPU; K = randn + a per-head offset.  Shared by every test: never modified."""
    lq, lk = LENGTHS[name]
    g = torch.Generator().manual_seed(SEEDS[name] + D + (1 if dt == BF16 else 0))
    q = torch.randn(sum(lq), HQ, D, generator=g).to(dt)
    k = (torch.randn(sum(lk), HK, D, generator=g) + torch.randn(1, HK, D, generator=g)).to(dt)
    v = torch.randn(sum(lk), HK, D, generator=g).to(dt)
    return q, k, v


@functools.lru_cache(maxsize=None)
def _oracle(name, D, dt, causal, sm_scale=None, smooth_k=True):
    from oracle import sage_oracle as O
    q, k, v = _inputs(name, D, dt)
    lq, lk = LENGTHS[name]
    return O.sageattn_varlen_oracle(q, k, v, _cu(lq), _cu(lk), is_causal=causal, sm_scale=sm_scale, smooth_k=smooth_k).float()


def _exact64(q, k, v, causal, sm_scale=None):
    """float64 attention of ONE sequence, q [M,Hq,D], k/v [N,Hk,D]; causal masks top-left (key j visible to row i iff
    j <= i, whatever M and N); no keys -> zeros.  A restatement of oracle.sdpa_fp32."""
    M, N = q.shape[0], k.shape[0]
    if N == 0:
        return torch.zeros(q.shape, dtype=torch.float64)
    g = q.shape[1] // k.shape[1]
    qh = q.double().transpose(0, 1)
    kh = k.double().transpose(0, 1).repeat_interleave(g, dim=0)
    vh = v.double().transpose(0, 1).repeat_interleave(g, dim=0)
    s = (qh @ kh.transpose(1, 2)) * (q.shape[-1] ** -0.5 if sm_scale is None else sm_scale)
    if causal:
        s = s.masked_fill(torch.arange(N).view(1, -1) > torch.arange(M).view(-1, 1), float("-inf"))
    return (torch.softmax(s, dim=-1) @ vh).transpose(0, 1)


def _exact_dev(name, D, dt, causal, o, sm_scale=None):
    """max over sequences of |o - exact float64 attention|"""
    q, k, v = _inputs(name, D, dt)
    lq, lk = LENGTHS[name]
    cq, ck = _cu(lq).tolist(), _cu(lk).tolist()
    worst = 0.0
    for s in range(len(lq)):
        r = _exact64(q[cq[s]:cq[s + 1]], k[ck[s]:ck[s + 1]], v[ck[s]:ck[s + 1]], causal, sm_scale)
        worst = max(worst, float((o[cq[s]:cq[s + 1]].double() - r).abs().max()))
    return worst


def _check_vs_oracle(o, oo, dt, what):
    """the suite's kernel-to-oracle bounds, unchanged; prints the figure first"""
    o = o.cpu().float()
    assert torch.isfinite(o).all(), what
    d = (o - oo).abs()
    if dt == F16:
        ulps = float((d / oo.abs().clamp(min=0.25)).max()) * 2.0 ** 10
        print(f"varlen-matrix {what}: fp16 max |o - oracle| = {ulps:.3f} x 2^-10 max(|oo|, 0.25), bound 4")
        assert (d <= 4 * 2.0 ** -10 * oo.abs().clamp(min=0.25)).all(), what
    else:
        print(f"varlen-matrix {what}: bf16 max |o - oracle| = {float(d.max()):.3e}, bound 1.6e-2")
        assert d.max() < 1.6e-2, what


def _call(name, D, dt, causal, nw, cu_dtype=torch.int32, max_q=None, max_k=None, tensors=None, **kw):
    """one sageattn_varlen call on the GPU with the wave override ``nw`` (0 = the dispatch rule), restored afterwards"""
    import sageattention_amd as sa
    from sageattention_amd import _lib as L
    q, k, v = tensors if tensors is not None else _inputs(name, D, dt)
    lq, lk = LENGTHS[name]
    args = (q.cuda(), k.cuda(), v.cuda(), _cu(lq, cu_dtype).cuda(), _cu(lk, cu_dtype).cuda(),
            max(lq) if max_q is None else max_q, max(lk) if max_k is None else max_k)
    assert L.lib().sage_set_tuning(0, nw) == 0
    try:
        o = sa.sageattn_varlen(*args, is_causal=causal, **kw)
        torch.cuda.synchronize()
    finally:
        L.lib().sage_set_tuning(0, 0)
    assert o.shape == q.shape and o.dtype == dt
    return o


DIMS = pytest.mark.parametrize("D", [64, 128])
DTYPES = pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
CAUSAL = pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])


# ---- 7. oracle anchor (CPU) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder", "cross"])
@DIMS
@DTYPES
@CAUSAL
def test_varlen_oracle_vs_exact_attention(name, D, dt, causal):
    """CPU: ``sageattn_varlen_oracle`` against float64 attention per sequence at 0.08 absolute, on the inputs of the length
    ladder and of the cross-length case: pins the oracle where no golden vector exists (causal with lq != lk: top-left).
    Measured maxima (the worse of fp16 / bf16) at head_dim 64 / 128: ladder full 0.0232 / 0.0204, ladder causal 0.0548 /
    0.0536 (rows with a handful of keys, where one INT8 step of a logit moves a large weight), cross full 0.0216 / 0.0287,
    cross causal 0.0363 / 0.0489."""
    dev = _exact_dev(name, D, dt, causal, _oracle(name, D, dt, causal))
    print(f"varlen-matrix oracle-anchor {name} D={D} {dt} causal={causal}: max |oracle - exact| = {dev:.4f}, bound 0.08")
    assert dev < 0.08


def test_varlen_oracle_keyless_sequence_is_zero_under_causal():
    """CPU: a sequence with queries and no keys gives zeros in the oracle, as in the float64 restatement, causal or not"""
    cq = _cu(LENGTHS["nokeys"][0]).tolist()
    for causal in (False, True):
        oo = _oracle("nokeys", 64, F16, causal)
        assert (oo[cq[1]:cq[2]] == 0).all()
        assert _exact_dev("nokeys", 64, F16, causal, oo) < 0.08


# ---- 1. length ladder ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@DIMS
@DTYPES
@CAUSAL
def test_varlen_length_ladder_every_geometry(D, dt, causal):
    """GPU: one packed call over the lengths 1 .. 449 around every multiple of 64 (sequences of 1-8 tiles; 64, 128, 192, 256,
    320 and 384 end on an aligned, unmasked last tile), with the dispatch rule's geometry, 4 waves and 8 waves: each within
    the oracle bound and finite, and the 4-wave and 8-wave outputs bit-identical."""
    oo = _oracle("ladder", D, dt, causal)
    outs = {}
    for nw in (0, 4, 8):
        outs[nw] = _call("ladder", D, dt, causal, nw).cpu()
        _check_vs_oracle(outs[nw], oo, dt, f"ladder D={D} causal={causal} nw={nw}")
    assert torch.equal(outs[4], outs[8]), (outs[4].float() - outs[8].float()).abs().max()
    assert torch.equal(outs[0], outs[4])  # at most 449 keys: the rule picks 4 waves


# ---- 2. cross lengths ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@DIMS
@DTYPES
@CAUSAL
@pytest.mark.parametrize("cu_dtype", [torch.int32, torch.int64], ids=["cu32", "cu64"])
def test_varlen_cross_lengths(D, dt, causal, cu_dtype):
    """GPU: q and k lengths differ in every sequence (more queries than keys, fewer, one key, one query), causal and not,
    4 and 8 waves, int32 and int64 cu_seqlens: against the oracle and, per sequence, exact attention with the top-left mask."""
    oo = _oracle("cross", D, dt, causal)
    outs = {}
    for nw in (4, 8):
        outs[nw] = _call("cross", D, dt, causal, nw, cu_dtype=cu_dtype).cpu()
        _check_vs_oracle(outs[nw], oo, dt, f"cross D={D} causal={causal} nw={nw} {cu_dtype}")
        dev = _exact_dev("cross", D, dt, causal, outs[nw])
        print(f"varlen-matrix cross D={D} {dt} causal={causal} nw={nw}: max |o - exact| = {dev:.4f}, bound 0.08")
        assert dev < 0.08
    assert torch.equal(outs[4], outs[8])


# ---- 3. the dispatch rule's own 8-wave choice ------------------------------------------------------------------------------
# attn_check (csrc/sage_attn.hip) receives max_seqlen_k as N and computes keys_per_row = is_causal ? N / 2 : N; with no
# override, fp16 PV (the only varlen form) and head_dim 128 it picks 4 waves iff keys_per_row <= 3072, else 8:
#   (a) N = 3136, non-causal:        keys_per_row = 3136 > 3072 -> 8 waves (the exact maxima of (b), N = 300, give 4)
#   (b) N = 4096, non-causal:        keys_per_row = 4096 > 3072 -> 8 waves
#       N = 8192, causal:            keys_per_row = 8192 / 2 = 4096 > 3072 -> 8 waves
@pytest.mark.gpu
@DTYPES
def test_varlen_dispatch_picks_8_waves_for_a_long_sequence(dt):
    """GPU, no override, head_dim 128: a packed batch with one sequence of 3136 keys (49 tiles) beside two short ones"""
    o = _call("long", 128, dt, False, 0)
    _check_vs_oracle(o, _oracle("long", 128, dt, False), dt, "dispatch-long D=128 nw=rule(8)")


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize("causal,max_k", [(False, 4096), (True, 8192)], ids=["full-4096", "causal-8192"])
def test_varlen_max_seqlen_upper_bounds(dt, causal, max_k):
    """GPU, no override, head_dim 128: ``max_seqlen_q`` = 512 and ``max_seqlen_k`` = a bucket size where the true maxima are
    300 -- the scale arrays and the grid are sized from them and the dispatch rule reads them (8 waves here, 4 for the exact
    maxima): bit-identical to the call with the exact maxima, and within the oracle bound."""
    exact = _call("cross", 128, dt, causal, 0)
    bucket = _call("cross", 128, dt, causal, 0, max_q=512, max_k=max_k)
    assert torch.equal(bucket, exact), (bucket.float() - exact.float()).abs().max()
    _check_vs_oracle(bucket, _oracle("cross", 128, dt, causal), dt, f"upper-bound D=128 causal={causal} max_k={max_k}")


# ---- 4. isolation ----------------------------------------------------------------------------------------------------------
def _poison(t):
    """a mix of NaN, +Inf and -Inf"""
    p = torch.full(t.shape, float("nan"), dtype=t.dtype)
    flat = p.view(-1)
    flat[1::3] = float("inf")
    flat[2::3] = float("-inf")
    return p


@pytest.mark.gpu
@DIMS
@CAUSAL
@pytest.mark.parametrize("nw", [4, 8])
def test_varlen_neighbour_sequence_cannot_leak(D, causal, nw):
    """GPU: the tile copies of sequence 0 (70 keys: its second tile spans rows 64..127) run on into sequence 1's rows, which
    must read as zero (per-sequence num_records; 0 * Inf would be NaN).  With the V rows of sequence 1 poisoned, and then its
    Q rows too, sequences 0 and 2 keep their bits.  (K stays finite: the smoothing mean spans all packed tokens.)"""
    q, k, v = _inputs("isolation", D, F16)
    lq, lk = LENGTHS["isolation"]
    cq, ck = _cu(lq).tolist(), _cu(lk).tolist()
    clean = _call("isolation", D, F16, causal, nw).cpu()
    _check_vs_oracle(clean, _oracle("isolation", D, F16, causal), F16, f"isolation D={D} causal={causal} nw={nw}")
    v_bad = v.clone()
    v_bad[ck[1]:ck[2]] = _poison(v[ck[1]:ck[2]])
    q_bad = q.clone()
    q_bad[cq[1]:cq[2]] = _poison(q[cq[1]:cq[2]])
    for tensors in ((q, k, v_bad), (q_bad, k, v_bad)):
        o = _call("isolation", D, F16, causal, nw, tensors=tensors).cpu()
        for s in (0, 2):
            assert torch.equal(o[cq[s]:cq[s + 1]], clean[cq[s]:cq[s + 1]]), (s, tensors[0] is q_bad)


# ---- 5. packed equals alone ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@DIMS
@DTYPES
@CAUSAL
def test_varlen_packed_equals_each_sequence_alone(D, dt, causal):
    """GPU, ``smooth_k=False`` (no mean couples the sequences): every sequence sent as its own one-sequence call returns the
    bits of its slice of the packed call, with 4 and with 8 waves."""
    import sageattention_amd as sa
    from sageattention_amd import _lib as L
    q, k, v = _inputs("cross", D, dt)
    lq, lk = LENGTHS["cross"]
    cq, ck = _cu(lq).tolist(), _cu(lk).tolist()
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    for nw in (4, 8):
        packed = _call("cross", D, dt, causal, nw, smooth_k=False)
        assert L.lib().sage_set_tuning(0, nw) == 0
        try:
            for s in range(len(lq)):
                one = sa.sageattn_varlen(qc[cq[s]:cq[s + 1]], kc[ck[s]:ck[s + 1]], vc[ck[s]:ck[s + 1]],
                                         _cu(lq[s:s + 1]).cuda(), _cu(lk[s:s + 1]).cuda(), lq[s], lk[s], is_causal=causal,
                                         smooth_k=False)
                assert torch.equal(one, packed[cq[s]:cq[s + 1]]), (nw, s)
        finally:
            L.lib().sage_set_tuning(0, 0)


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@DIMS
@DTYPES
@CAUSAL
def test_varlen_sm_scale_and_no_smoothing(D, dt, causal):
    """GPU: ``sm_scale = 0.05`` and ``smooth_k=False`` (K keeps its per-head offset) against the oracle, 4 and 8 waves"""
    oo = _oracle("cross", D, dt, causal, 0.05, False)
    for nw in (4, 8):
        o = _call("cross", D, dt, causal, nw, sm_scale=0.05, smooth_k=False)
        _check_vs_oracle(o, oo, dt, f"sm_scale=0.05 smooth_k=False D={D} causal={causal} nw={nw}")


@pytest.mark.gpu
@DIMS
@pytest.mark.parametrize("nw", [8, 4])
def test_varlen_keyless_sequence_under_causal(D, nw):
    """GPU: the no-keys case of test_varlen.py (200 queries without keys between two ordinary sequences), causal: with 8 waves
    the zero fill covers 256-row q-blocks.  The output block is pre-filled with NaN through the caching allocator; the keyless
    rows are 0 and all other rows within the oracle bound."""
    lq, _ = LENGTHS["nokeys"]
    cq = _cu(lq).tolist()
    q, k, v = (t.cuda() for t in _inputs("nokeys", D, F16))
    poison = torch.full((sum(lq), HQ, D), float("nan"), dtype=F16, device="cuda")
    del poison  # its block is the next allocation of that size: the operator's output
    o = _call("nokeys", D, F16, True, nw, tensors=(q, k, v))
    assert torch.isfinite(o).all()
    assert (o[cq[1]:cq[2]] == 0).all()
    _check_vs_oracle(o, _oracle("nokeys", D, F16, True), F16, f"keyless causal D={D} nw={nw}")
