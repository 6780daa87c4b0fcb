"""Block-sparse attention on the GPU.  The gate is bit-identity: a sparse call that visits tiles {t1 < ... < tk} performs the
arithmetic of the dense kernel run on those tiles gathered into one contiguous K/V, in the same order.  Then the oracle, the
masked operator the feature replaces, plan reuse, capture / compile and map views."""
import ctypes

import pytest
import torch

from blocksparse_util import expand_map, gather_block, make_map

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    return sageattention_amd


def _hnd(x, layout):
    return x if layout == "HND" else x.transpose(1, 2)


def _alloc(layout, B, H, n, D, dtype, gen):
    """randn in the given memory layout, returned as its [B,H,n,D] view"""
    shape = (B, H, n, D) if layout == "HND" else (B, n, H, D)
    return _hnd(torch.randn(shape, generator=gen).to(dtype).cuda(), layout)


def _desc(L, t):
    return L.SageTensor(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))


def _lists(sa, bm, M, N):
    return sa.block_sparse_plan(bm.cuda(), M, N).lists


def _attn_q8(L, sparse, pv_fp8, q8, k8, v, o, qs, ks, v_scale, lse, M, N, gran, lists=None):
    """sage_attn_qk_int8_pv_{f16,f8}[_blocksparse] on [B,H,n,D] views (raw base-2 LSE)"""
    B, Hq, _, D = q8.shape
    Hk = k8.shape[1]
    head = (_desc(L, q8), _desc(L, k8), _desc(L, v))
    odt = L.dtype_code(o.dtype)
    mid = (_desc(L, o), odt, qs.data_ptr(), ks.data_ptr())
    tail = (None, lse.data_ptr(), B, Hq, Hk, M, N, D, 0, gran, 128, 32, D ** -0.5, 0)
    if pv_fp8:
        args = head + mid + (v_scale.data_ptr(),) + tail
        name = "sage_attn_qk_int8_pv_f8"
    else:
        args = head + (L.dtype_code(v.dtype),) + mid + tail
        name = "sage_attn_qk_int8_pv_f16"
    if sparse:
        name += "_blocksparse"
        args += (lists.data_ptr(), lists.numel() * 4)
    L.check(getattr(L.lib(), name)(*args, L.stream_ptr(q8.device)), name)


def _structured_map(B, Hq, nqb, ntk):
    """List lengths 1, 2, odd, even, longer than the four-slot ring and full; the ragged last tile on and off; rotated
    per head so that every q-block position meets several lengths."""
    rows = []
    rows.append([3 % ntk])                                  # one tile
    rows.append([0, ntk - 1])                               # two, the last (ragged) tile on
    rows.append([1, 4 % ntk, ntk - 2])                      # odd, last tile off
    rows.append([0, 2, 5 % ntk, ntk - 1])                   # even, last tile on
    rows.append(sorted({0, 1, 3, 6 % ntk, 7 % ntk, 8 % ntk, ntk - 2}))  # longer than the ring, last off
    rows.append(list(range(ntk)))                           # everything
    rows.append(sorted({2, 3, 4, 5 % ntk, 9 % ntk, ntk - 1}))
    bm = torch.zeros(B, Hq, nqb, ntk, dtype=torch.bool)
    for b in range(B):
        for h in range(Hq):
            for i in range(nqb):
                bm[b, h, i, rows[(i + h + 2 * b) % len(rows)]] = True
    return bm


# (D, v kind, granularity, layout, B, Hq, Hk, M, N)
_BIT_CASES = []
for _i, (_D, _v, _g) in enumerate((D, v, g) for D in (64, 128) for v in ("fp16", "bf16", "fp8") for g in ("per_warp", "per_thread")):
    _BIT_CASES.append((_D, _v, _g, "HND" if _i % 2 == 0 else "NHD", 1 + _i % 2, 4, 2, 128 * 5 + 50, 64 * 11 + 37))
_BIT_CASES += [(64, "fp16", "per_thread", "NHD", 1, 2, 2, 256, 512),      # no ragged tile, M != N
               (128, "fp8", "per_thread", "HND", 1, 2, 1, 700, 700),      # M == N
               (128, "bf16", "per_warp", "HND", 1, 4, 4, 356, 64 * 20)]   # lists of up to 20 tiles, no ragged tile


@pytest.mark.parametrize("case", _BIT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_bit_identical_to_the_dense_kernel_on_gathered_tiles(sa, case):
    """For EVERY (b, h, q-block): gather the active K rows, k scales and V tiles into contiguous tensors, run the existing
    dense int8-Q entry point on that 128-row block: torch.equal on o and on the raw base-2 LSE."""
    from sageattention_amd import _lib as L, core
    from sageattention_amd.quant import per_channel_fp8
    D, vkind, gran, layout, B, Hq, Hk, M, N = case
    gen = torch.Generator().manual_seed(sum(x for x in case if isinstance(x, int)) + len(case[1]) + len(case[2]))
    dtype = torch.bfloat16 if vkind == "bf16" else torch.float16
    q, k, v = (_alloc(layout, B, H, n, D, dtype, gen) for H, n in ((Hq, M), (Hk, N), (Hk, N)))
    nat = lambda x: _hnd(x, layout)  # noqa: E731  (the tensor as the layout-aware helpers of the package expect it)
    k8, ks, km = core._prep_k(nat(k), layout, gran, True)
    q8, qs, _ = core._quant_q(nat(q), km, layout, gran, D ** -0.5, 32, False, Hq, Hk)
    q8, k8 = _hnd(q8, layout), _hnd(k8, layout)
    pv_fp8 = vkind == "fp8"
    v_scale = None
    if pv_fp8:
        v8, v_scale, _ = per_channel_fp8(nat(v), tensor_layout=layout, scale_max=448.0, smooth_v=False)
        vv = v8 if layout == "HND" else v8.transpose(1, 2)  # [B,Hk,D,Npad]
    else:
        vv = v
    nqb, ntk = (M + 127) // 128, (N + 63) // 64
    bm = _structured_map(B, Hq, nqb, ntk)
    lists = _lists(sa, bm, M, N)
    code = core._GRAN_CODE[gran]
    o = _hnd(torch.full((B, Hq, M, D) if layout == "HND" else (B, M, Hq, D), float("nan"), dtype=dtype, device="cuda"), layout)
    lse = torch.full((B, Hq, M), float("nan"), device="cuda")
    _attn_q8(L, True, pv_fp8, q8, k8, vv, o, qs, ks, v_scale, lse, M, N, code, lists)
    torch.cuda.synchronize()
    per_k = 4 if gran == "per_thread" else 1
    per_q = 32 if gran == "per_thread" else 4
    assert L.lib().sage_set_tuning(0, 4) == 0
    try:
        for b in range(B):
            for h in range(Hq):
                hk = h // (Hq // Hk)
                for i in range(nqb):
                    r0, r1 = 128 * i, min(128 * i + 128, M)
                    tiles = torch.nonzero(bm[b, h, i]).flatten()
                    cols = gather_block(bm[b, h, i], N).cuda()
                    Ng = cols.numel()
                    k8g = k8[b:b + 1, hk:hk + 1, cols].contiguous()
                    ksg = ks[b, hk].view(ntk, per_k)[tiles.cuda()].contiguous().view(1, 1, -1)
                    if pv_fp8:
                        tcols = (tiles.view(-1, 1) * 64 + torch.arange(64).view(1, 64)).flatten().cuda()
                        vg = vv[b:b + 1, hk:hk + 1][..., tcols].contiguous()
                        vsg = v_scale[b:b + 1, hk:hk + 1].contiguous()
                    else:
                        vg, vsg = vv[b:b + 1, hk:hk + 1, cols].contiguous(), None
                    q8g = q8[b:b + 1, h:h + 1, r0:r1].contiguous()
                    qsg = qs[b, h, per_q * i:per_q * (i + 1)].contiguous().view(1, 1, -1)
                    og = torch.empty(1, 1, r1 - r0, D, dtype=dtype, device="cuda")
                    lg = torch.empty(1, 1, r1 - r0, device="cuda")
                    _attn_q8(L, False, pv_fp8, q8g, k8g, vg, og, qsg, ksg, vsg, lg, r1 - r0, Ng, code)
                    torch.cuda.synchronize()
                    assert torch.equal(o[b, h, r0:r1], og[0, 0]), (b, h, i, tiles.tolist())
                    assert torch.equal(lse[b, h, r0:r1], lg[0, 0]), (b, h, i, tiles.tolist())
    finally:
        L.lib().sage_set_tuning(0, 0)


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("gran", ["per_warp", "per_thread"])
def test_all_ones_map_is_the_dense_operator(sa, pv, D, gran):
    """An all-ones map is bit-identical to the dense operator on the whole tensor: the fused-Q form through the public
    functions (o and the final LSE), the int8-Q form through the C ABI (o and the raw base-2 LSE)."""
    from sageattention_amd import _lib as L, core
    from sageattention_amd.quant import per_channel_fp8
    torch.manual_seed(D + len(gran))
    B, Hq, Hk, M, N = 2, 4, 2, 700, 1000
    q, k, v = (torch.randn(B, H, n, D, dtype=torch.float16, device="cuda") for H, n in ((Hq, M), (Hk, N), (Hk, N)))
    ones = torch.ones(1, 1, (M + 127) // 128, (N + 63) // 64, dtype=torch.bool, device="cuda")
    dense = sa.sageattn_qk_int8_pv_fp16_cuda if pv == "fp16" else sa.sageattn_qk_int8_pv_fp8_cuda
    assert L.lib().sage_set_tuning(0, 4) == 0  # the dense operator in the sparse kernel's geometry, whatever the dispatch rule
    try:
        o_d, l_d = dense(q, k, v, qk_quant_gran=gran, return_lse=True, pv_accum_dtype="fp32")
    finally:
        L.lib().sage_set_tuning(0, 0)
    o_s, l_s = sa.sageattn_block_sparse(q, k, v, ones, pv=pv, qk_quant_gran=gran, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o_s, o_d) and torch.equal(l_s, l_d)
    k8, ks, km = core._prep_k(k, "HND", gran, True)
    q8, qs, _ = core._quant_q(q, km, "HND", gran, D ** -0.5, 32, False, Hq, Hk)
    vv, v_scale = v, None
    if pv == "fp8":
        vv, v_scale, _ = per_channel_fp8(v, tensor_layout="HND", scale_max=448.0, smooth_v=False)
    lists = sa.block_sparse_plan(ones, M, N, B=B, Hq=Hq).lists
    outs = []
    assert L.lib().sage_set_tuning(0, 4) == 0
    try:
        for sparse in (False, True):
            o = torch.empty_like(q)
            lse = torch.empty(B, Hq, M, device="cuda")
            _attn_q8(L, sparse, pv == "fp8", q8, k8, vv, o, qs, ks, v_scale, lse, M, N, core._GRAN_CODE[gran], lists)
            outs.append((o, lse))
    finally:
        L.lib().sage_set_tuning(0, 0)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _oracle(q, k, v, bm, layout, pv, gran, sm_scale=None):
    """The operator composed from the oracle's parts, as tests/test_masked.py composes the masked one."""
    from oracle import sage_oracle as O
    D = q.shape[-1]
    sm_scale = D ** -0.5 if sm_scale is None else sm_scale
    km = O.k_mean(k, layout)
    quant = O.per_thread_int8 if gran == "per_thread" else O.per_warp_int8
    q8, qs, k8, ks = quant(q, k, km, tensor_layout=layout)
    q8h, k8h = O._to_hnd(q8, layout), O._to_hnd(k8, layout)
    M, N = q8h.shape[2], k8h.shape[2]
    qrows, kcols = O.expand_q_scale(qs, M, gran), O.expand_k_scale(ks, N, gran)
    E = expand_map(bm.expand(q8h.shape[0], q8h.shape[1], -1, -1), M, N)
    if pv == "fp16":
        vh = O._to_hnd(v, layout)
        o, lse2 = O.attn_tile_loop(q8h, k8h, vh, qrows, kcols, logit_mult=sm_scale * LOG2E, out_dtype=q.dtype, attn_mask=E)
    else:
        v8, v_scale, _ = O.per_channel_fp8(v, tensor_layout=layout, smooth_v=False)
        v8h = v8 if layout == "HND" else v8.transpose(1, 2)
        o, lse2 = O.attn_tile_loop(q8h, k8h, v8h, qrows, kcols, logit_mult=sm_scale * LOG2E, pv="fp8", v_scale=v_scale,
                                   out_dtype=q.dtype, attn_mask=E)
    lse = lse2 / LOG2E + O.lse_correction(q, km, layout) * sm_scale
    return O._from_hnd(o, layout), lse


_TOL = {("fp16", torch.float16): 2e-3, ("fp16", torch.bfloat16): 1.6e-2, ("fp8", torch.float16): 0.06,
        ("fp8", torch.bfloat16): 0.07}
_LSE_TOL = 3e-3


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("cfg", [("HND", 64, "per_thread", 1, 4, 2, 300, 333), ("NHD", 128, "per_warp", 2, 2, 2, 513, 1027),
                                 ("NHD", 64, "per_warp", 1, 3, 1, 640, 200), ("HND", 128, "per_thread", 1, 2, 1, 130, 2048)],
                         ids=lambda c: "-".join(map(str, c)))
def test_end_to_end_vs_oracle(sa, pv, dt, cfg):
    """sageattn_block_sparse against the oracle's tile loop on the expanded map; every q-block of these maps has an active
    tile, so EVERY row is compared.  Tolerances of the dense edge-shape and random-sweep tests on the same kind of data."""
    layout, D, gran, B, Hq, Hk, M, N = cfg
    g = torch.Generator().manual_seed(M * 1000 + N)
    mk = (lambda h, n: (B, h, n, D)) if layout == "HND" else (lambda h, n: (B, n, h, D))
    q, k, v = (torch.randn(mk(H, n), generator=g).to(dt) for H, n in ((Hq, M), (Hk, N), (Hk, N)))
    bm = make_map(B, Hq, M, N, density=0.4, seed=N)
    assert bm.any(-1).all()
    o, lse = sa.sageattn_block_sparse(q.cuda(), k.cuda(), v.cuda(), bm.cuda(), tensor_layout=layout, pv=pv,
                                      qk_quant_gran=gran, return_lse=True)
    torch.cuda.synchronize()
    oo, ol = _oracle(q, k, v, bm, layout, pv, gran)
    assert o.shape == q.shape and o.dtype == dt
    do, dl = (o.cpu().float() - oo.float()).abs().max().item(), (lse.cpu() - ol).abs().max().item()
    print(f"block-sparse vs oracle {cfg} {pv} {dt}: |do| {do:.3e} |dlse| {dl:.3e}")
    assert do < _TOL[(pv, dt)]
    assert dl < _LSE_TOL


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_empty_q_blocks_are_defined(sa, pv, D):
    """Rows of a q-block without any active tile: exactly o = 0 and lse = -inf (the masked operator leaves such rows
    undefined); the other rows against the oracle."""
    torch.manual_seed(7)
    B, Hq, Hk, M, N = 2, 2, 1, 128 * 3 + 20, 500
    q, k, v = (torch.randn(B, H, n, D).half() for H, n in ((Hq, M), (Hk, N), (Hk, N)))
    bm = make_map(B, Hq, M, N, density=0.5, seed=1)
    bm[0, 0, 1] = False
    bm[1, 1, 3] = False   # the partial last q-block
    bm[1, 0, 0] = False
    o, lse = sa.sageattn_block_sparse(q.cuda(), k.cuda(), v.cuda(), bm.cuda(), pv=pv, return_lse=True)
    o_only = sa.sageattn_block_sparse(q.cuda(), k.cuda(), v.cuda(), bm.cuda(), pv=pv)
    torch.cuda.synchronize()
    rows_on = expand_map(bm, M, N).any(-1)  # [B,Hq,M]
    assert (~rows_on).sum() == 128 + 20 + 128
    assert (o.cpu()[~rows_on] == 0).all() and (lse.cpu()[~rows_on] == float("-inf")).all()
    assert torch.equal(o_only, o)
    oo, ol = _oracle(q, k, v, bm, "HND", pv, "per_thread")
    assert (o.cpu().float() - oo.float())[rows_on].abs().max() < _TOL[(pv, torch.float16)]
    assert (lse.cpu() - ol)[rows_on].abs().max() < _LSE_TOL
    assert torch.isfinite(o).all()


@pytest.mark.parametrize("D", [64, 128])
def test_agrees_with_the_masked_operator(sa, D):
    """FP16 PV: the expanded bool mask through sageattn_qk_int8_pv_fp16_triton (the path this feature replaces; per-thread
    scales, the serial masked loop) agrees within the FP16-PV tolerance."""
    torch.manual_seed(D)
    B, Hq, Hk, M, N = 1, 4, 2, 400, 777
    q, k, v = (torch.randn(B, H, n, D, dtype=torch.float16, device="cuda") for H, n in ((Hq, M), (Hk, N), (Hk, N)))
    bm = make_map(B, Hq, M, N, density=0.3, seed=D).cuda()
    o_s, l_s = sa.sageattn_block_sparse(q, k, v, bm, pv="fp16", return_lse=True)
    o_m, l_m = sa.sageattn_qk_int8_pv_fp16_triton(q, k, v, attn_mask=expand_map(bm, M, N), return_lse=True)
    torch.cuda.synchronize()
    assert (o_s.float() - o_m.float()).abs().max() < 2e-3
    assert (l_s - l_m).abs().max() < _LSE_TOL


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_plan_reuse_and_determinism(sa, pv):
    torch.manual_seed(3)
    B, Hq, Hk, M, N, D = 2, 4, 4, 1000, 1500, 128
    bm = make_map(B, Hq, M, N, density=0.35, seed=9).cuda()
    plan = sa.block_sparse_plan(bm, M, N)
    assert torch.equal(plan.lists, sa.block_sparse_plan(bm, M, N).lists)  # the compaction itself is deterministic
    first = None
    for step in range(3):  # new inputs, the same plan
        q, k, v = (torch.randn(B, Hq, n, D, dtype=torch.float16, device="cuda") for n in (M, N, N))
        a = sa.sageattn_block_sparse(q, k, v, plan, pv=pv, return_lse=True)
        b = sa.sageattn_block_sparse(q, k, v, bm, pv=pv, return_lse=True)
        c = sa.sageattn_block_sparse(q, k, v, plan, pv=pv, return_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
        first = first if first is not None else a[0]
    assert not torch.equal(first, a[0])


def test_compact_lists_format(sa):
    """count, ascending tiles, then the last tile repeated to the end of the row (an empty row: zeros)."""
    B, Hq, M, N = 1, 2, 300, 64 * 70 + 1
    bm = make_map(B, Hq, M, N, density=0.5, seed=2)
    bm[0, 1, 2] = False
    lists = sa.block_sparse_plan(bm.cuda(), M, N).lists.cpu()
    ntk = 71
    row = (1 + ntk + 5 + 3) // 4 * 4
    lists = lists.view(B, Hq, 3, row)
    for h in range(Hq):
        for i in range(3):
            on = torch.nonzero(bm[0, h, i]).flatten().tolist()
            r = lists[0, h, i].tolist()
            assert r[0] == len(on) and r[1:1 + len(on)] == on
            assert r[1 + len(on):] == [on[-1] if on else 0] * (row - 1 - len(on))
            assert row - 1 - len(on) >= 5


@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_compiles_as_one_graph_and_captures(sa, pv):
    """The op traces under torch.compile(fullgraph=True) and records into a HIP graph (map or plan), bit-identical to eager."""
    import sageattention_amd.ops as ops
    torch.manual_seed(0)
    B, Hq, Hk, M, N, D = 1, 4, 2, 384, 640, 128
    q, k, v = (torch.randn(B, H, n, D, dtype=torch.float16, device="cuda") for H, n in ((Hq, M), (Hk, N), (Hk, N)))
    bm = make_map(B, Hq, M, N, density=0.5, seed=4).cuda()
    plan = sa.block_sparse_plan(bm, M, N)

    def block(q, k, v, bm):
        return ops.sageattn_block_sparse_compilable(q * 1.0, k, v, bm, pv=pv) + 1.0

    def block_plan(q, k, v):
        return ops.sageattn_block_sparse_compilable(q * 1.0, k, v, plan, pv=pv) + 1.0

    want = sa.sageattn_block_sparse(q, k, v, bm, pv=pv)
    ran = []
    for backend in ("aot_eager", "inductor"):
        try:
            got = torch.compile(block, backend=backend, fullgraph=True)(q, k, v, bm)
            got_p = torch.compile(block_plan, backend=backend, fullgraph=True)(q, k, v)
        except torch._dynamo.exc.BackendCompilerFailed:
            if backend == "inductor":   # no usable code generator for the surrounding pointwise ops on this machine
                continue               # (tests/test_custom_op.py treats the dense op the same way)
            raise
        assert torch.equal(got, want + 1.0) and torch.equal(got_p, want + 1.0), backend
        ran.append(backend)
    print(f"attn_block_sparse[{pv}] compiled with fullgraph=True under: {ran}")
    assert "aot_eager" in ran
    for arg in (bm, plan):
        for _ in range(2):
            sa.sageattn_block_sparse(q, k, v, arg, pv=pv, return_lse=True)  # warm up: module load, function attributes
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            o_g, l_g = sa.sageattn_block_sparse(q, k, v, arg, pv=pv, return_lse=True)
        for seed in (2, 3):
            torch.manual_seed(seed)
            q.copy_(torch.randn_like(q)); k.copy_(torch.randn_like(k)); v.copy_(torch.randn_like(v))
            g.replay()
            torch.cuda.synchronize()
            o_e, l_e = sa.sageattn_block_sparse(q, k, v, arg, pv=pv, return_lse=True)
            assert torch.equal(o_g, o_e) and torch.equal(l_g, l_e)


def test_map_views(sa):
    """A non-contiguous or broadcast view of the map gives the result of its contiguous copy."""
    torch.manual_seed(1)
    B, Hq, Hk, M, N, D = 2, 4, 2, 500, 900, 64
    q, k, v = (torch.randn(B, H, n, D, dtype=torch.float16, device="cuda") for H, n in ((Hq, M), (Hk, N), (Hk, N)))
    nqb, ntk = 4, 15
    big = (torch.rand(B, 2 * nqb, Hq, 3 * ntk + 1, generator=torch.Generator().manual_seed(5)) < 0.4)
    big[..., 1] = True
    big = big.cuda()
    views = [big[:, ::2, :, 1::3].transpose(1, 2),                      # strided in every dimension, heads and rows swapped
             big[:1, :nqb, :1, :ntk].transpose(1, 2),                   # broadcast over batch and heads: [1,1,nqb,ntk]
             big[:, :nqb, :1, :ntk].transpose(1, 2).expand(B, Hq, nqb, ntk),  # broadcast over heads with 0 stride
             big[:, :nqb, :, :ntk].transpose(1, 2).to(torch.uint8)]     # uint8
    for view in views:
        assert tuple(view.shape[2:]) == (nqb, ntk)
        full = view.expand(B, Hq, nqb, ntk).contiguous()
        assert full.any(-1).all()
        a = sa.sageattn_block_sparse(q, k, v, view, return_lse=True)
        b = sa.sageattn_block_sparse(q, k, v, full, return_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(sa.sageattn_block_sparse(q, k, v, views[0]), sa.sageattn_block_sparse(q, k, v, views[1]))
