"""The INT8 quantizers after their vector-instruction diet (profiles/k_quant_valu_diet.md) against the CPU oracle
(oracle/sage_oracle.py: k_mean, per_block_int8, per_thread_int8, per_warp_int8), which shares no code with them: every
int8 value and the bits of every scale EQUAL, no element left out.  The shapes are the smallest that reach each path the
diet changed: the streaming K quantizer with several blocks per workgroup and a ragged last block, the
one-block-per-workgroup kernel in every run-time form it keeps (Q and K, mult != 1), tensors made of rounding ties
(the exact-division fallback for every element), a single row.

Inputs lie on a grid of 1/16 with |x| <= 32, so a column sum over <= 1100 rows is exact in fp32 in ANY order: the mean of
the two-pass reduction on the GPU and the oracle's are the same bits, and the comparison needs no tolerance anywhere."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def sa():
    assert torch.cuda.is_available()
    import sageattention_amd
    return sageattention_amd


def _grid_tensor(shape, dt, seed):
    """randn * 2 plus a per-channel offset of up to +-4 standard deviations, on a grid of 1/16 (module docstring).  With
    the offset a row past the end of the sequence (zeros, or whatever a kernel reads there) becomes -mean after the
    subtraction, several times the largest centred value: it would dominate the maxima if it leaked into them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.round(torch.randn(shape, generator=g) * 32) / 16
    off = torch.round((torch.rand((1, 1, 1, shape[-1]), generator=g) * 16 - 8) * 16) / 16
    return (x.clamp(-8, 8) + off).to(dt)


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _assert_same(got8, gots, ref8, refs, what):
    refs = refs.reshape(gots.shape)
    assert torch.equal(_bits(gots), _bits(refs)), (what, "scales", int((_bits(gots) != _bits(refs)).sum()))
    assert torch.equal(got8.cpu(), ref8), (what, "int8", int((got8.cpu() != ref8).sum()))


# ---- the streaming kernel: several blocks per workgroup, ragged tail -------------------------------------------------------

# B*H*ceil(N/64) = 1440 > 1024 workgroups (head_dim 128) and 1536 > 1280 (head_dim 64): two blocks per workgroup; N % 64 != 0
STREAM_SHAPES = [(2, 40, 1100, 128), (3, 32, 1000, 64)]


@functools.lru_cache(maxsize=None)
def _stream_case(shape, dtname):
    """K and the oracle's results for the three (granularity, rounding) forms of a dense K call, computed once."""
    from oracle import sage_oracle as O
    k = _grid_tensor(shape, DTYPES[dtname], 1000 + shape[2])
    q = torch.zeros((1, 1, 8, shape[-1]), dtype=k.dtype)
    km = O.k_mean(k)
    ref = {"km": km.squeeze(2)}
    _, _, ref["pt8"], ref["pts"] = O.per_thread_int8(q, k, km=km)
    _, _, ref["pbt8"], ref["pbts"] = O.per_block_int8(q, k, km=km, rounding="triton")
    _, _, ref["pbc8"], ref["pbcs"] = O.per_block_int8(q, k, km=km, rounding="cuda")
    return k, ref


@pytest.mark.parametrize("form", ["per_thread_triton", "per_block_triton", "per_block_cuda"])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_streaming_k_quantizer_equals_the_oracle(sa, shape, dtname, form):
    from sageattention_amd import _lib as L
    from sageattention_amd.quant import k_smooth_quant
    k, ref = _stream_case(shape, dtname)
    gran, rnd, key = {"per_thread_triton": (L.GRAN_PER_THREAD, L.ROUND_TRITON, "pt"),
                      "per_block_triton": (L.GRAN_PER_BLOCK, L.ROUND_TRITON, "pbt"),
                      "per_block_cuda": (L.GRAN_PER_BLOCK, L.ROUND_CUDA, "pbc")}[form]
    k8, ks, km = k_smooth_quant(k.cuda(), "HND", gran, rnd)
    assert torch.equal(km.cpu().view(torch.int16), ref["km"].view(torch.int16)), "km"
    _assert_same(k8, ks, ref[key + "8"], ref[key + "s"], (shape, dtname, form))


def test_streaming_k_quantizer_single_row(sa):
    """(2, 48, 1, 64): the last block is the first block, the mean is the row and k - km is all zeros (scale 0 or 1e-7)."""
    from oracle import sage_oracle as O
    from sageattention_amd import _lib as L
    from sageattention_amd.quant import k_smooth_quant
    for dtname, dt in DTYPES.items():
        k = _grid_tensor((2, 48, 1, 64), dt, 77)
        q = torch.zeros((1, 1, 8, 64), dtype=dt)
        km = O.k_mean(k)
        for gran, rnd, ref in ((L.GRAN_PER_THREAD, L.ROUND_TRITON, O.per_thread_int8(q, k, km=km)[2:]),
                               (L.GRAN_PER_BLOCK, L.ROUND_TRITON, O.per_block_int8(q, k, km=km, rounding="triton")[2:]),
                               (L.GRAN_PER_BLOCK, L.ROUND_CUDA, O.per_block_int8(q, k, km=km, rounding="cuda")[2:])):
            k8, ks, kmg = k_smooth_quant(k.cuda(), "HND", gran, rnd)
            assert torch.equal(kmg.cpu().view(torch.int16), km.squeeze(2).view(torch.int16))
            _assert_same(k8, ks, ref[0], ref[1], (dtname, gran, rnd))


# ---- the one-block-per-workgroup kernel keeps its run-time forms ------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(1, 2, 130, 128), (2, 3, 65, 64)], ids=lambda s: "x".join(map(str, s)))
def test_general_quantizer_equals_the_oracle(sa, shape, dtname):
    """Q and K, blocks of 64 and 128, the three granularities, both roundings, and the Q multiplier sm_scale * log2 e of
    the per_block form: the mult == 1 / is_key / 64-row specialisation of the streaming kernel must not reach this one."""
    from oracle import sage_oracle as O
    from sageattention_amd import _lib as L
    from sageattention_amd.quant import _quant
    dt = DTYPES[dtname]
    q, k = _grid_tensor(shape, dt, 5), _grid_tensor(shape, dt, 6)
    km = O.k_mean(k)
    qd, kd, kmd = q.cuda(), k.cuda(), km.squeeze(2).contiguous().cuda()
    sm_scale = shape[-1] ** -0.5
    mult = sm_scale * O.LOG2E
    assert abs(mult - 1.0) > 0.5
    for blkq in (64, 128):
        for blkk in (64, 128):
            for rounding, rnd in (("triton", L.ROUND_TRITON), ("cuda", L.ROUND_CUDA)):
                rq8, rqs, rk8, rks = O.per_block_int8(q, k, km=km, BLKQ=blkq, BLKK=blkk, sm_scale=sm_scale, rounding=rounding)
                q8, qs, _ = _quant(qd, "HND", L.GRAN_PER_BLOCK, False, blkq, blkq, mult, rnd)
                k8, ks, _ = _quant(kd, "HND", L.GRAN_PER_BLOCK, True, blkk, blkk, 1.0, rnd, mean=kmd)
                _assert_same(q8, qs, rq8, rqs, ("per_block Q", blkq, rounding))
                _assert_same(k8, ks, rk8, rks, ("per_block K", blkk, rounding))
            for warpq in (16, 32):
                rq8, rqs, rk8, rks = O.per_warp_int8(q, k, km=km, BLKQ=blkq, WARPQ=warpq, BLKK=blkk)
                q8, qs, _ = _quant(qd, "HND", L.GRAN_PER_WARP, False, blkq, warpq, 1.0, L.ROUND_CUDA)
                k8, ks, _ = _quant(kd, "HND", L.GRAN_PER_BLOCK, True, blkk, blkk, 1.0, L.ROUND_CUDA, mean=kmd)
                _assert_same(q8, qs, rq8, rqs, ("per_warp Q", blkq, warpq))
                _assert_same(k8, ks, rk8, rks, ("per_warp K", blkk))
                rq8, rqs, rk8, rks = O.per_thread_int8(q, k, km=km, BLKQ=blkq, WARPQ=warpq, BLKK=blkk, WARPK=64)
                q8, qs, _ = _quant(qd, "HND", L.GRAN_PER_THREAD, False, blkq, warpq, 1.0, L.ROUND_TRITON)
                k8, ks, _ = _quant(kd, "HND", L.GRAN_PER_THREAD, True, blkk, 64, 1.0, L.ROUND_TRITON, mean=kmd)
                _assert_same(q8, qs, rq8, rqs, ("per_thread Q", blkq, warpq))
                _assert_same(k8, ks, rk8, rks, ("per_thread K", blkk))


# ---- rounding ties -------------------------------------------------------------------------------------------------------

def _tie_tensor(dt):
    """(1, 1, 128, 64): every value a half-integer in [-126.5, 126.5] except one +127 and one -127 per 64-row block.  Row
    63 - r of a block is minus row r, so every column sums to zero exactly: the mean is 0 and k - km is k.  With one scale
    per block and the Triton form the scale is 127 / 127 = 1 and EVERY element sits on a rounding boundary."""
    g = torch.Generator().manual_seed(9)
    blocks = []
    for _ in range(2):
        top = (torch.randint(0, 127, (32, 64), generator=g).float() + 0.5) * (torch.randint(0, 2, (32, 64), generator=g) * 2 - 1)
        top[:16, :2] = (torch.arange(0, 127, 4)[:32].float().view(16, 2) + 0.5)  # a spread of magnitudes for certain
        top[0, 0], top[31, 63] = 126.5, -126.5
        top[5, 7] = 127.0
        blocks.append(torch.cat([top, -top.flip(0)], 0))
    x = torch.cat(blocks, 0).view(1, 1, 128, 64)
    assert (x.sum(2) == 0).all() and x.abs().max() == 127 and ((x.abs() % 1 == 0.5).sum() == x.numel() - 4)
    assert torch.equal(x.to(dt).float(), x)  # every value is representable (bf16: <= 8 significant bits)
    return x.to(dt)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_rounding_ties_go_through_the_exact_division(sa, dtname):
    from oracle import sage_oracle as O
    from sageattention_amd import _lib as L
    from sageattention_amd.quant import _quant, k_smooth_quant
    k = _tie_tensor(DTYPES[dtname])
    q = torch.zeros((1, 1, 8, 64), dtype=k.dtype)
    refs = {(L.GRAN_PER_BLOCK, L.ROUND_TRITON): O.per_block_int8(q, k, rounding="triton")[2:],
            (L.GRAN_PER_BLOCK, L.ROUND_CUDA): O.per_block_int8(q, k, rounding="cuda")[2:],
            (L.GRAN_PER_THREAD, L.ROUND_TRITON): O.per_thread_int8(q, k)[2:]}
    # what the oracle is expected to say: scale exactly 1, half away from zero (Triton) / ties to even (CUDA)
    r8, rs = refs[(L.GRAN_PER_BLOCK, L.ROUND_TRITON)]
    kf = k.float()
    assert (rs == 1.0).all() and torch.equal(r8.float(), torch.where(kf.abs() == 127, kf, kf + 0.5 * kf.sign()))
    r8, rs = refs[(L.GRAN_PER_BLOCK, L.ROUND_CUDA)]
    assert (rs == 1.0).all() and torch.equal(r8.float(), torch.round(kf))
    for (gran, rnd), (ref8, refs_) in refs.items():
        k8, ks, _ = _quant(k.cuda(), "HND", gran, True, 64, 64, 1.0, rnd, mean=None)  # no mean subtraction
        _assert_same(k8, ks, ref8, refs_, ("general", gran, rnd))
        k8, ks, km = k_smooth_quant(k.cuda(), "HND", gran, rnd)  # the streaming kernel: the mean is exactly zero
        assert (km == 0).all()
        _assert_same(k8, ks, ref8, refs_, ("streaming", gran, rnd))
