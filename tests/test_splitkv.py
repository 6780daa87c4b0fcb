"""Split-KV attention (``sageattn_splitkv``, ``sage_attn_fusedq_pv_{f16,f8}_splitkv``) without a GPU: the key ranges of the rule
partition the tiles, the automatic split count, the Python refusals, the C status table of the two entry points and the
torch.library ops.  What the kernels compute: test_splitkv_gpu.py."""
import pytest
import torch

import splitkv_util as SU


# ---- 1. the ranges of the rule ---------------------------------------------------------------------------------------------
def test_ranges_partition_the_tiles():
    """for every (len, S): the splits' ranges are consecutive, cover [0, ntk) exactly, the non-empty ones come first, and
    their number is ceil(ntk / tps)"""
    for n in range(0, 1101, 37):
        ntk = (n + 63) // 64
        for S in range(1, SU.SPLITKV_MAX + 1):
            ranges = [SU.split_range(n, S, s) for s in range(S)]
            nxt, nonempty, seen_empty = 0, 0, False
            for t0, t1 in ranges:
                if t0 < t1:
                    assert not seen_empty and t0 == nxt, (n, S, ranges)
                    nxt, nonempty = t1, nonempty + 1
                else:
                    seen_empty = True
            assert nxt == ntk, (n, S, ranges)
            tps = -(-ntk // S)
            assert nonempty == SU.nonempty_splits(n, S) == (-(-ntk // tps) if ntk else 0), (n, S)
            assert nonempty <= S and (nonempty > 0) == (n > 0)


def test_range_map_columns():
    bm = SU.range_map([1000, 65, 0], 1000, 200, 4, 3, 1)
    assert bm.shape == (3, 4, 2, 16)
    assert bm[0, 0, 0].nonzero().flatten().tolist() == list(range(6, 12))   # 16 tiles, tps 6
    assert bm[1, 3, 1].nonzero().flatten().tolist() == [1]                  # 2 tiles, tps 1
    assert not bm[2].any()


# ---- 2. the automatic choice -----------------------------------------------------------------------------------------------
def test_num_splits_rule():
    from sageattention_amd import core
    import sageattention_amd as sa
    assert sa.splitkv_num_splits is core.splitkv_num_splits
    for B, Hq, M, N in [(1, 40, 512, 32760), (1, 32, 128, 65536), (8, 8, 4, 8192), (4, 32, 8192, 8192), (2, 4, 200, 1000),
                        (1, 1, 1, 1), (1, 1, 1, 1 << 17), (16, 32, 1, 100), (1, 512, 1, 4096), (3, 7, 129, 513)]:
        S = core.splitkv_num_splits(B, Hq, M, N)
        grid, ntk = B * Hq * ((M + 127) // 128), (N + 63) // 64
        assert 1 <= S <= 16 and S <= max(1, -(-ntk // 8)), (B, Hq, M, N, S)
        if grid >= 512:
            assert S == 1, (B, Hq, M, N, S)
        assert S == max(1, min(16, -(-ntk // 8), -(-512 // grid)))
    assert core.splitkv_num_splits(1, 40, 512, 32760) == 4
    assert core.splitkv_num_splits(1, 32, 128, 65536) == 16
    assert core.splitkv_num_splits(4, 32, 8192, 8192) == 1


# ---- 3. Python refusals, raised before any device call -----------------------------------------------------------------------
def test_python_refusals():
    import sageattention_amd as sa
    from sageattention_amd import core
    import sageattention
    assert "sageattn_splitkv" in sa.__all__ and "sageattn_splitkv" in core.__all__ and sa.sageattn_splitkv is core.sageattn_splitkv
    assert sageattention.sageattn_splitkv is core.sageattn_splitkv and sageattention.core.sageattn_splitkv is core.sageattn_splitkv
    q = torch.zeros(2, 4, 70, 64, dtype=torch.float16)
    k = torch.zeros(2, 2, 1000, 64, dtype=torch.float16)
    lens = torch.tensor([1000, 7], dtype=torch.int32)
    for kw in (dict(is_causal=True), dict(attn_mask=torch.ones(70, 1000, dtype=torch.bool)), dict(smooth_k=False),
               dict(smooth_v=True), dict(block_map=torch.ones(1, 1, 1, 16, dtype=torch.bool)),
               dict(cu_seqlens_q=torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError, match="does not take"):
            sa.sageattn_splitkv(q, k, k, num_splits=2, **kw)
    with pytest.raises(TypeError, match="unexpected keyword"):
        sa.sageattn_splitkv(q, k, k, num_splits=2, window=3)
    with pytest.raises(TypeError, match="int32"):
        sa.sageattn_splitkv(q, k, k, lens.long(), 2)
    with pytest.raises(TypeError, match="kv_lens"):
        sa.sageattn_splitkv(q, k, k, [1000, 7], 2)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="kv_lens shape"):
            sa.sageattn_splitkv(q, k, k, bad, 2)
    with pytest.raises(ValueError, match="is on"):
        sa.sageattn_splitkv(q, k, k, lens.to("meta"), 2)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="num_splits"):
            sa.sageattn_splitkv(q, k, k, num_splits=bad)
    with pytest.raises(TypeError, match="num_splits"):
        sa.sageattn_splitkv(q, k, k, num_splits=2.0)
    with pytest.raises(ValueError, match="pv"):
        sa.sageattn_splitkv(q, k, k, num_splits=2, pv="int8")
    with pytest.raises(ValueError, match="qk_quant_gran"):
        sa.sageattn_splitkv(q, k, k, num_splits=2, qk_quant_gran="per_block")
    with pytest.raises(ValueError, match="layout"):
        sa.sageattn_splitkv(q, k, k, num_splits=2, tensor_layout="BHSD")
    with pytest.raises(ValueError, match="one shape"):
        sa.sageattn_splitkv(q, k, k[..., :32], lens, 2, pv="fp8")
    with pytest.raises(AssertionError, match="cuda"):  # as every operator of the package on CPU tensors
        sa.sageattn_splitkv(q, k, k, lens, 2)


# ---- 4. the C status table ---------------------------------------------------------------------------------------------------
# Fake device addresses: where a GPU is visible a missed check would launch kernels on them, so this runs only where none
# is; there every launch attempt returns SAGE_ERR_LAUNCH (-5), which makes a launch observable (tests/test_cabi_symbols.py).
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")

FAKE = 1 << 20
_PARAMS = {
    "sage_attn_fusedq_pv_f16_splitkv": "q qdt k v vdt o odt ks km vm lse B Hq Hk M N D gran warpq sm lens S ws wsb stream",
    "sage_attn_fusedq_pv_f8_splitkv": "q qdt k v o odt ks km vs vm lse B Hq Hk M N D gran warpq sm lens S ws wsb stream",
}
_B, _HQ, _M, _D, _S = 2, 2, 200, 64, 5
_NEED = _S * _B * _HQ * _M * (_D + 1) * 4


def _call(fn, **change):
    from sageattention_amd import _lib as L
    t = L.SageTensor(FAKE, 1 << 16, 1 << 12, 64)
    args = dict(q=t, k=t, v=t, o=t, vdt=0, odt=0, qdt=0, ks=FAKE, vs=FAKE, vm=None, km=FAKE, lse=None, B=_B, Hq=_HQ, Hk=1, M=_M,
                N=333, D=_D, gran=3, warpq=32, sm=0.125, lens=FAKE, S=_S, ws=FAKE, wsb=_NEED, stream=None)
    args.update(change)
    return getattr(L.lib(), fn)(*[args[n] for n in _PARAMS[fn].split()])


def test_workspace_bytes():
    from sageattention_amd import _lib as L
    f = L.lib().sage_splitkv_workspace_bytes
    assert f(_B, _HQ, _M, _D, _S) == _NEED and f(1, 1, 1, 128, 16) == 16 * 129 * 4
    assert [f(*a) for a in ((0, 1, 1, 64, 2), (1, 1, 1, 64, 0), (1, 1, 1, 64, 17), (1, 1, 0, 64, 2))] == [0, 0, 0, 0]


@no_gpu
def test_valid_calls_reach_a_launch():
    for fn in _PARAMS:
        assert _call(fn) == -5
        assert _call(fn, lens=None, lse=FAKE, S=1, qdt=1, odt=1) == -5
        assert _call(fn, S=16, wsb=16 * _B * _HQ * _M * (_D + 1) * 4, gran=2) == -5


@no_gpu
def test_status_table():
    """Each argument made invalid on its own returns its argument status: nothing was launched (a launch returns -5 here)."""
    cases = []
    for fn in _PARAMS:
        cases += [(fn, dict(S=0), -1), (fn, dict(S=17), -1), (fn, dict(S=-1), -1), (fn, dict(ws=None), -1),
                  (fn, dict(ws=FAKE + 8), -1), (fn, dict(wsb=_NEED - 1), -1), (fn, dict(wsb=0), -1), (fn, dict(lens=FAKE + 2), -1),
                  (fn, dict(gran=1), -3), (fn, dict(km=None), -3), (fn, dict(km=FAKE + 8), -3), (fn, dict(vm=FAKE), -3),
                  (fn, dict(N=1 << 25), -4), (fn, dict(D=96), -2), (fn, dict(N=0), -1), (fn, dict(B=0), -1), (fn, dict(M=0), -1),
                  (fn, dict(ks=None), -1), (fn, dict(sm=0.0), -1), (fn, dict(Hk=3), -1), (fn, dict(qdt=2), -1),
                  (fn, dict(odt=2), -1), (fn, dict(gran=0), -1), (fn, dict(q=None), -1), (fn, dict(o=None), -1)]
    cases += [("sage_attn_fusedq_pv_f8_splitkv", dict(vs=None), -1), ("sage_attn_fusedq_pv_f16_splitkv", dict(vdt=2), -1)]
    wrong = [(fn, sorted(c), st, got) for fn, c, st in cases if (got := _call(fn, **c)) != st]
    assert not wrong, wrong


# ---- 5. the torch.library ops ----------------------------------------------------------------------------------------------
def test_op_schemas_and_fake_shapes():
    import sageattention_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    want = ("Tensor q, Tensor k, Tensor v, Tensor? kv_lens, SymInt num_splits, str tensor_layout, float sm_scale, str pv, "
            "str qk_quant_gran")
    s, s_lse = (str(getattr(torch.ops.sageattention_amd, n).default._schema) for n in ("attn_splitkv", "attn_splitkv_lse"))
    assert want in s and s.endswith("-> Tensor")
    assert want in s_lse and s_lse.endswith("-> (Tensor, Tensor)")
    assert "sageattn_splitkv_compilable" in ops.__all__
    with FakeTensorMode():
        for layout, shp, kshp in (("HND", (3, 8, 70, 72), (3, 4, 1000, 72)), ("NHD", (3, 70, 8, 72), (3, 1000, 4, 72))):
            q = torch.empty(shp, dtype=torch.bfloat16, device="cuda")
            k = torch.empty(kshp, dtype=torch.bfloat16, device="cuda")
            lens = torch.empty((3,), dtype=torch.int32, device="cuda")
            o = ops.sageattn_splitkv_compilable(q, k, k, lens, 4, tensor_layout=layout, pv="fp8")
            assert o.shape == q.shape and o.dtype == q.dtype and o.device == q.device and o.is_contiguous()
            o, lse = ops.sageattn_splitkv_compilable(q, k, k, tensor_layout=layout, return_lse=True)
            assert o.shape == q.shape and lse.shape == (3, 8, 70) and lse.dtype == torch.float32
    with pytest.raises(ValueError, match="layout"):
        ops.sageattn_splitkv_compilable(torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64),
                                        tensor_layout="BHSD")
    with pytest.raises(ValueError, match="num_splits"):
        ops.sageattn_splitkv_compilable(torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64),
                                        num_splits=17)
