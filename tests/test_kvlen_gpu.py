"""Per-batch key lengths on the GPU (``sageattn_kvlen``; the rule: include/sageattn_hip.h, per-batch key lengths).

The reference for batch b is the existing public operator on the slice -- ``sageattn_qk_int8_pv_fp16_cuda`` or
``sageattn_qk_int8_pv_fp8_cuda`` on ``q[b:b+1]`` and the first len_b keys, same granularity, ``return_lse=True``, on the same
GPU -- and the comparison is ``torch.equal`` on o and lse: the rule admits no tolerance.  In every case the K and V rows
>= len_b hold NaN, so anything that reads them -- a statistic of the pre-pass, a tile copy, a V row times P = 0 -- shows.
Hq = 4 on Hk = 2 (GQA) and M = 200 (one full and one ragged 128-row q-block) unless a case says otherwise."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HQ, HK, M = 4, 2, 200
NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    import sageattention_amd.ops  # noqa: F401  (registers the ops)
    return sageattention_amd


def _make(B, N, D, dtype=torch.float16, seed=0, m=M, layout="HND"):
    """seeded q, k, v on the GPU; k carries a per-channel offset, so that the smoothing mean matters"""
    g = torch.Generator().manual_seed(1000 * D + N + seed)
    q = torch.randn(B, HQ, m, D, generator=g)
    k = torch.randn(B, HK, N, D, generator=g) + 2.0 * torch.randn(B, HK, 1, D, generator=g)
    v = torch.randn(B, HK, N, D, generator=g)
    q, k, v = (t.to(dtype).cuda() for t in (q, k, v))
    if layout == "NHD":
        q, k, v = (t.transpose(1, 2).contiguous() for t in (q, k, v))
    return q, k, v


def _clamped(lens, N):
    return [min(max(int(x), 0), N) for x in lens]


def _poison(k, v, lens, layout="HND"):
    """NaN into the K and V rows >= len_b"""
    for b, n in enumerate(lens):
        if layout == "HND":
            k[b, :, n:] = float("nan")
            v[b, :, n:] = float("nan")
        else:
            k[b, n:] = float("nan")
            v[b, n:] = float("nan")


def _keys(t, b, n, layout):
    return t[b:b + 1, :, :n] if layout == "HND" else t[b:b + 1, :n]


def _check(sa, q, k, v, lens, pv, gran, causal=False, layout="HND"):
    """sageattn_kvlen against the dense operator on every batch's slice, bit for bit; a batch without keys: o = 0, lse = -inf"""
    N = k.size(2) if layout == "HND" else k.size(1)
    eff = _clamped(lens, N)
    _poison(k, v, eff, layout)
    dense = sa.sageattn_qk_int8_pv_fp16_cuda if pv == "fp16" else sa.sageattn_qk_int8_pv_fp8_cuda
    kv_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    o, lse = sa.sageattn_kvlen(q, k, v, kv_lens, tensor_layout=layout, is_causal=causal, pv=pv, qk_quant_gran=gran,
                               return_lse=True)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == q.dtype and lse.shape == (q.size(0), HQ, q.size(2 if layout == "HND" else 1))
    for b, n in enumerate(eff):
        if n == 0:
            assert torch.equal(o[b], torch.zeros_like(o[b])), f"batch {b}: o of a batch without keys"
            assert torch.equal(lse[b], torch.full_like(lse[b], NEG_INF)), f"batch {b}: lse of a batch without keys"
            continue
        ro, rl = dense(q[b:b + 1], _keys(k, b, n, layout), _keys(v, b, n, layout), tensor_layout=layout, is_causal=causal,
                       qk_quant_gran=gran, return_lse=True)
        torch.cuda.synchronize()
        assert torch.isfinite(ro.float()).all() and torch.isfinite(rl).all()
        assert torch.equal(o[b:b + 1], ro), f"batch {b} (len {n}): o differs in {int((o[b:b + 1] != ro).sum())} elements"
        assert torch.equal(lse[b:b + 1], rl), f"batch {b} (len {n}): lse differs in {int((lse[b:b + 1] != rl).sum())} rows"
    return o, lse


# ---- 1. tile and chunk edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gran", ["per_thread", "per_warp"])
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_tile_and_chunk_edges(sa, D, pv, gran):
    """N = 320 (five tiles; two chunks of 256 rows): a full batch, one row into the last tile and the second chunk (257), a
    whole number of tiles and of chunks (256), one row into the second tile (65), a single key, none"""
    lens = [320, 257, 256, 65, 1, 0]
    q, k, v = _make(len(lens), 320, D)
    _check(sa, q, k, v, lens, pv, gran)


def test_bf16(sa):
    lens = [320, 257, 65, 0]
    q, k, v = _make(len(lens), 320, 128, dtype=torch.bfloat16)
    _check(sa, q, k, v, lens, "fp16", "per_thread")
    q, k, v = _make(len(lens), 320, 64, dtype=torch.bfloat16, seed=1)
    _check(sa, q, k, v, lens, "fp8", "per_warp")


# ---- 2. pre-pass chunk-size switch and the 8-wave geometry ------------------------------------------------------------------
LONG = [4400, 4097, 4096, 3073, 300]


@pytest.mark.parametrize("D,pv,gran", [(128, "fp16", "per_thread"), (128, "fp16", "per_warp"), (64, "fp8", "per_thread")])
def test_chunk_size_switch_and_geometry(sa, D, pv, gran):
    """N = 4400: chunks of 512 rows above 4096 rows, of 256 up to there (16 chunks at 4096, more than the 9 of 4400), and at
    head_dim 128 with FP16 PV 8-wave workgroups above 3072 keys per row.  The padded call picks its geometry and grids from
    N, each sliced call from its len_b (300 keys: 4 waves), and the bits still agree."""
    q, k, v = _make(len(LONG), 4400, D)
    _check(sa, q, k, v, LONG, pv, gran)


# ---- 3. causal ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_causal(sa, D, pv):
    """top-left aligned: N = M = 320; with 200 and 64 keys the rows beyond them see all the keys of their batch"""
    lens = [320, 200, 64]
    q, k, v = _make(len(lens), 320, D, m=320)
    _check(sa, q, k, v, lens, pv, "per_thread", causal=True)


# ---- 4. NHD layout and a head_dim that is padded -----------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_nhd_head_dim_72(sa, pv):
    lens = [200, 77, 1, 0]
    q, k, v = _make(len(lens), 200, 72, layout="NHD")
    o, _ = _check(sa, q, k, v, lens, pv, "per_thread", layout="NHD")
    assert o.shape == (len(lens), M, HQ, 72)


# ---- 5. lengths outside [0, N] -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_lengths_are_clamped(sa, pv):
    """N + 5 behaves as N and -3 as 0"""
    N = 130
    q, k, v = _make(2, N, 64)
    o, lse = _check(sa, q, k, v, [N + 5, -3], pv, "per_thread")
    o2, lse2 = sa.sageattn_kvlen(q, k, v, torch.tensor([N, 0], dtype=torch.int32, device="cuda"), pv=pv, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


# ---- 6. the pre-pass alone ---------------------------------------------------------------------------------------------------
def _check_prepass(k, v, lens, gran):
    """NaN into the K and V rows >= len_b, then ``k_smooth_quant_kvlen`` and ``kv_prepare_fp8_kvlen`` against the calls without
    lengths on every batch's slice: km, the INT8 K rows < len_b and their scales, v_scale and the V^T bytes up to the padded
    length equal, bit for bit; zero bytes in the pad columns of the last 64-token block; km = 0 for a batch without keys"""
    from sageattention_amd import core, quant
    _poison(k, v, lens)
    kv_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    kg, rnd = core._k_pairing(gran)
    per = 4 if gran == "per_thread" else 1
    k8, ks, km = quant.k_smooth_quant_kvlen(k, kv_lens, "HND", kg, rnd)
    f8, fs, fm, v8, vs = quant.kv_prepare_fp8_kvlen(k, v, kv_lens, "HND", kg, rnd)
    torch.cuda.synchronize()
    order = quant.fp8_token_order().cuda()
    for b, n in enumerate(lens):
        if n == 0:
            assert torch.equal(km[b], torch.zeros_like(km[b])) and torch.equal(fm[b], torch.zeros_like(fm[b]))
            continue
        nb, npad = (n + 63) // 64, (n + 63) // 64 * 64
        r8, rs, rm = quant.k_smooth_quant(k[b:b + 1, :, :n], "HND", kg, rnd)
        g8, gs, gm, w8, ws = quant.kv_prepare_fp8(k[b:b + 1, :, :n], v[b:b + 1, :, :n], "HND", kg, rnd)
        torch.cuda.synchronize()
        for name, got, ref in (("km", km[b:b + 1], rm), ("k8", k8[b:b + 1, :, :n], r8), ("k_scale", ks[b:b + 1, :, :nb * per], rs),
                               ("km (fp8)", fm[b:b + 1], gm), ("k8 (fp8)", f8[b:b + 1, :, :n], g8),
                               ("k_scale (fp8)", fs[b:b + 1, :, :nb * per], gs), ("v_scale", vs[b:b + 1], ws),
                               ("v_fp8", v8[b:b + 1, :, :, :npad].view(torch.uint8), w8.view(torch.uint8))):
            assert torch.equal(got, ref), f"{name} of batch {b} (len {n})"
        assert torch.isfinite(rm.float()).all() and torch.isfinite(rs).all() and torch.isfinite(ws).all()
        beyond = order + 64 * (nb - 1) >= n  # positions of the last 64-token block that hold tokens >= len_b
        last = v8[b, :, :, npad - 64:npad].view(torch.uint8)
        assert not last[..., beyond].any(), f"V^T pad columns of batch {b} (len {n})"


@pytest.mark.parametrize("N,lens", [(320, [320, 257, 256, 65, 1, 0]), (4400, LONG)], ids=["n320", "n4400"])
@pytest.mark.parametrize("gran", ["per_thread", "per_warp"])
@pytest.mark.parametrize("D", [64, 128])
def test_prepass(sa, D, gran, N, lens):
    """km, the INT8 K rows < len_b and their scales, and for FP8 v_scale and the V^T columns < len_b, equal those of the
    pre-pass called on the slice; the V^T columns up to the end of the last 64-token block are zero bytes; km of a batch
    without keys is 0"""
    _, k, v = _make(len(lens), N, D, seed=2)
    _check_prepass(k, v, lens, gran)


def _kv(B, H, N, D, dtype, seed):
    """seeded k and v of H heads, drawn on the GPU (the streaming shapes are up to 126 MB an operand); k with a per-channel
    offset as in _make"""
    g = torch.Generator(device="cuda").manual_seed(1000 * D + N + seed)
    k = torch.randn(B, H, N, D, generator=g, device="cuda") + 2.0 * torch.randn(B, H, 1, D, generator=g, device="cuda")
    v = torch.randn(B, H, N, D, generator=g, device="cuda")
    return k.to(dtype), v.to(dtype)


# The smallest shapes at which the dense K/V pre-pass streams (test_gpu_parity.py): by units_per_wg a V workgroup walks 4 units
# at head_dim 64 and 16 at 128 (streaming from 4 and 12), a K workgroup of sage_k_smooth_quant 4 blocks at head_dim 64
STREAMING = [((4, 32, 2050, 64), [2050, 2049, 1300, 0]), ((3, 40, 4100, 128), [4100, 4097, 65])]


@pytest.mark.parametrize("gran", ["per_thread", "per_warp"])  # (per_thread, triton) and (per_block, cuda)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape,lens", STREAMING, ids=["d64", "d128"])
def test_prepass_streaming(sa, shape, lens, dtype, gran):
    """test_prepass where the calls with lengths run the streaming kernels, K and V, several blocks per workgroup; the sliced
    calls (one batch) do not stream, and the two dense forms are held equal in test_gpu_parity.py"""
    k, v = _kv(*shape, dtype, seed=5)
    _check_prepass(k, v, lens, gran)


@pytest.mark.parametrize("dtype,gran", [(torch.float16, "per_thread"), (torch.bfloat16, "per_warp")], ids=["fp16-per_thread", "bf16-per_warp"])
@pytest.mark.parametrize("shape", [(2, 2, 320, 64), (2, 2, 4400, 128), STREAMING[0][0]], ids=["n320", "n4400", "streaming"])
def test_full_lengths_take_the_other_branch_of_one_text(sa, shape, dtype, gran):
    """kv_lens = [N] * B: every output equals that of the call without lengths on the same operands -- km, k8, scales, v_scale
    and all V^T bytes, pad columns included.  (2, 2, 4400, 128): 16 chunk slots per head for 9 chunks, so the workspace is
    addressed through part_shift"""
    from sageattention_amd import core, quant
    B, _, N, _ = shape
    k, v = _kv(*shape, dtype, seed=6)
    kv_lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    kg, rnd = core._k_pairing(gran)
    got = quant.k_smooth_quant_kvlen(k, kv_lens, "HND", kg, rnd) + quant.kv_prepare_fp8_kvlen(k, v, kv_lens, "HND", kg, rnd)
    ref = quant.k_smooth_quant(k, "HND", kg, rnd) + quant.kv_prepare_fp8(k, v, "HND", kg, rnd)
    torch.cuda.synchronize()
    names = ("k8", "k_scale", "km", "k8 (fp8)", "k_scale (fp8)", "km (fp8)", "v_fp8", "v_scale")
    for name, a, r in zip(names, got, ref):
        a, r = (t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t for t in (a, r))
        assert torch.equal(a, r), name
    assert all(torch.isfinite(t.float()).all() for t in ref if t.dtype != torch.float8_e4m3fn)


# ---- 7. HIP-graph capture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_graph_capture_reads_the_lengths_at_replay(sa, pv):
    """one captured call, kv_lens overwritten in place, replay: the output of an eager call with the new lengths"""
    first, second = [320, 100, 7], [64, 320, 0]
    q, k, v = _make(3, 320, 64, seed=3)
    _poison(k, v, [max(a, b) for a, b in zip(first, second)])
    kv_lens = torch.tensor(first, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sa.sageattn_kvlen(q, k, v, kv_lens, pv=pv, return_lse=True)  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og, lg = sa.sageattn_kvlen(q, k, v, kv_lens, pv=pv, return_lse=True)
    for lens in (second, first):
        kv_lens.copy_(torch.tensor(lens, dtype=torch.int32))
        og.fill_(1.0); lg.zero_()
        graph.replay()
        oe, le = sa.sageattn_kvlen(q, k, v, torch.tensor(lens, dtype=torch.int32, device="cuda"), pv=pv, return_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(og, oe) and torch.equal(lg, le), lens
        assert torch.isfinite(og.float()).all()


# ---- 8. torch.compile ----------------------------------------------------------------------------------------------------------
def test_compile_fullgraph(sa):
    from sageattention_amd.ops import sageattn_kvlen_compilable
    lens = [320, 130, 0]
    q, k, v = _make(3, 320, 128, seed=4)
    _poison(k, v, lens)
    kv_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    o, lse = sa.sageattn_kvlen(q, k, v, kv_lens, pv="fp8", return_lse=True)
    oe, le = sageattn_kvlen_compilable(q, k, v, kv_lens, pv="fp8", return_lse=True)
    fn = torch.compile(lambda a, b, c, n: sageattn_kvlen_compilable(a, b, c, n, pv="fp8", return_lse=True), fullgraph=True)
    oc, lc = fn(q, k, v, kv_lens)
    torch.cuda.synchronize()
    assert torch.equal(oe, o) and torch.equal(le, lse) and torch.equal(oc, o) and torch.equal(lc, lse)
    assert torch.equal(o[2], torch.zeros_like(o[2])) and torch.isfinite(o.float()).all()
