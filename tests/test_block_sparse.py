"""Block-sparse attention without a GPU: the reference the GPU tests use is sound, the C-ABI entry points check every
argument before their first launch, the list sizing, the Python-level errors and the fake implementation of the op."""
import ctypes

import pytest
import torch

from blocksparse_util import expand_map, gather_block, make_map


# ---- 1. the reference of the GPU tests ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_masked_oracle_equals_dense_oracle_on_gathered_tiles(pv):
    """oracle.attn_tile_loop(attn_mask = the block map expanded to [B,H,M,N]) is the reference for every row with an active
    block.  Pinned here against the DENSE oracle run per q-block on the active tiles gathered into one contiguous K/V:
    bit-equal o and base-2 LSE (the -1e6 terms of leading masked tiles are annihilated exactly by the later rescale).
    Ragged N = 333, M = 300, the first tile off in every row, the ragged last tile on in some rows and off in others."""
    from oracle import sage_oracle as O
    torch.manual_seed(5)
    B, Hq, Hk, M, N, D = 1, 2, 1, 300, 333, 64
    q, k, v = torch.randn(B, Hq, M, D).half(), torch.randn(B, Hk, N, D).half(), torch.randn(B, Hk, N, D).half()
    km = O.k_mean(k)
    q8, qs, k8, ks = O.per_thread_int8(q, k, km)
    qrows, kcols = O.expand_q_scale(qs, M, "per_thread"), O.expand_k_scale(ks, N, "per_thread")
    mult = D ** -0.5 * 1.4426950408889634
    bm = make_map(B, Hq, M, N, density=0.5, seed=3)
    bm[..., 0] = False
    bm[0, 0, :, -1] = torch.tensor([True, False, True])
    bm[0, 1, :, -1] = torch.tensor([False, True, False])
    bm[..., 2] |= ~bm.any(-1)  # every q-block keeps a tile
    assert bm.any(-1).all() and not bm[..., 0].any()
    kw = dict(logit_mult=mult, pv=pv)
    if pv == "fp8":
        vv, v_scale, _ = O.per_channel_fp8(v, smooth_v=False)
        kw["v_scale"] = v_scale
    else:
        vv = v
    o, lse2 = O.attn_tile_loop(q8, k8, vv, qrows, kcols, attn_mask=expand_map(bm, M, N), **kw)
    for h in range(Hq):
        for i in range((M + 127) // 128):
            r0, r1 = 128 * i, min(128 * i + 128, M)
            cols = gather_block(bm[0, h, i], N)
            hk = h // (Hq // Hk)
            vg = vv[:, hk:hk + 1, :, cols] if pv == "fp8" else vv[:, hk:hk + 1, cols]
            kwg = dict(kw, v_scale=kw["v_scale"][:, hk:hk + 1]) if pv == "fp8" else kw
            og, lg = O.attn_tile_loop(q8[:, h:h + 1, r0:r1], k8[:, hk:hk + 1, cols], vg, qrows[:, h:h + 1, r0:r1],
                                      kcols[:, hk:hk + 1, cols], **kwg)
            assert (o[:, h:h + 1, r0:r1].float() - og.float()).abs().max() == 0.0, (h, i)
            assert (lse2[:, h:h + 1, r0:r1] - lg).abs().max() == 0.0, (h, i)


# ---- 2. every argument is checked before the first launch -------------------------------------------------------------
# Fake device addresses: where a GPU is visible a missed check would launch kernels on them, so this runs only where none
# is; there every launch attempt returns SAGE_ERR_LAUNCH (-5), which makes a launch observable (tests/test_cabi_symbols.py).
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")

FAKE = 1 << 20
ODD = FAKE + 8

_PARAMS = {
    "sage_block_map_compact": "map mstr B Hq M N lists nbytes stream",
    "sage_attn_qk_int8_pv_f16_blocksparse":
        "q k v vdt o odt qs ks vm lse B Hq Hk M N D causal gran blkq warpq sm lm1 lists nbytes stream",
    "sage_attn_qk_int8_pv_f8_blocksparse":
        "q k v o odt qs ks vs vm lse B Hq Hk M N D causal gran blkq warpq sm lm1 lists nbytes stream",
    "sage_attn_fusedq_pv_f16_blocksparse": "q qdt k v vdt o odt ks km vm lse B Hq Hk M N D causal gran warpq sm lists nbytes stream",
    "sage_attn_fusedq_pv_f8_blocksparse": "q qdt k v o odt ks km vs vm lse B Hq Hk M N D causal gran warpq sm lists nbytes stream",
}
_ATTN = [fn for fn in _PARAMS if "attn" in fn]


def _valid(fn):
    from sageattention_amd import _lib as L
    t = L.SageTensor(FAKE, 1 << 16, 1 << 12, 64)
    B, Hq, M, N = 1, 2, 200, 333
    nbytes = L.lib().sage_block_sparse_workspace_bytes(B, Hq, M, N)
    if fn == "sage_block_map_compact":
        return dict(map=FAKE, mstr=(ctypes.c_int64 * 4)(0, 12, 6, 1), B=B, Hq=Hq, M=M, N=N, lists=FAKE, nbytes=nbytes, stream=None)
    return dict(q=t, k=t, v=t, vdt=0, o=t, odt=0, qs=FAKE, ks=FAKE, vs=FAKE, vm=None, lse=None, B=B, Hq=Hq, Hk=1, M=M, N=N,
                D=64, causal=0, gran=3, blkq=128, warpq=32, sm=0.125, lm1=0, qdt=0, km=FAKE, lists=FAKE, nbytes=nbytes,
                stream=None)


def _call(fn, **change):
    from sageattention_amd import _lib as L
    args = dict(_valid(fn), **change)
    return getattr(L.lib(), fn)(*[args[n] for n in _PARAMS[fn].split()])


@no_gpu
def test_valid_calls_reach_a_launch():
    assert [fn for fn in _PARAMS if _call(fn) != -5] == []


@no_gpu
def test_single_fault_status_table():
    """Each argument made invalid on its own returns its argument status: nothing was launched (a launch returns -5 here)."""
    from sageattention_amd import _lib as L
    need = _valid(_ATTN[0])["nbytes"]
    cases = [("sage_block_map_compact", c, -1) for c in (
        dict(map=None), dict(lists=None), dict(lists=ODD), dict(mstr=None), dict(mstr=(ctypes.c_int64 * 4)(0, 12, -6, 1)),
        dict(nbytes=need - 4), dict(nbytes=0), dict(B=0), dict(Hq=0), dict(M=0), dict(N=0))]
    for fn in _ATTN:
        cases += [(fn, dict(lists=None), -1), (fn, dict(lists=ODD), -1), (fn, dict(nbytes=need - 4), -1),
                  (fn, dict(nbytes=0), -1), (fn, dict(D=96), -2), (fn, dict(causal=1), -3), (fn, dict(vm=FAKE), -3),
                  (fn, dict(sm=0.0), -1), (fn, dict(sm=-1.0), -1), (fn, dict(sm=float("nan")), -1),
                  (fn, dict(q=L.SageTensor(ODD, 1 << 16, 1 << 12, 64)), -1), (fn, dict(ks=None), -1), (fn, dict(Hk=3), -1),
                  (fn, dict(N=1 << 25, nbytes=1 << 40), -4)]
    # a list buffer sized for fewer keys than the call has
    small = L.lib().sage_block_sparse_workspace_bytes(1, 2, 200, 64)
    cases += [(fn, dict(nbytes=small), -1) for fn in _ATTN]
    wrong = [(fn, sorted(c), st, got) for fn, c, st in cases if (got := _call(fn, **c)) != st]
    assert not wrong, wrong


# ---- 3. sizing ---------------------------------------------------------------------------------------------------------
def test_workspace_bytes():
    """One row per (b, h_q, 128-row q-block): 1 count + ceil(N/64) tiles + 5 pad entries, rounded up to 4 int32."""
    from sageattention_amd import _lib as L
    f = L.lib().sage_block_sparse_workspace_bytes
    assert f(1, 2, 300, 333) == 2 * 3 * 12 * 4            # 1 + 6 + 5 = 12
    assert f(4, 32, 8192, 8192) == 4 * 32 * 64 * 136 * 4  # 1 + 128 + 5 = 134 -> 136
    assert f(1, 1, 1, 1) == 8 * 4
    assert f(0, 1, 64, 64) == 0 and f(1, 1, 0, 64) == 0 and f(1, 1, 64, -1) == 0


# ---- 4. Python-level errors, raised before any device call ------------------------------------------------------------
def test_python_errors():
    import sageattention_amd as sa
    import sageattention_amd.ops  # noqa: F401  (registers the ops)
    q = torch.zeros(1, 2, 300, 64, dtype=torch.float16)
    k = torch.zeros(1, 2, 333, 64, dtype=torch.float16)
    good = torch.ones(1, 2, 3, 6, dtype=torch.bool)
    with pytest.raises(ValueError, match="non-causal"):
        sa.sageattn_block_sparse(q, k, k, good, is_causal=True)
    with pytest.raises(TypeError, match="dtype"):
        sa.sageattn_block_sparse(q, k, k, good.float())
    with pytest.raises(TypeError):
        sa.sageattn_block_sparse(q, k, k, None)
    for bad in (torch.ones(1, 2, 3, 5, dtype=torch.bool), torch.ones(1, 2, 2, 6, dtype=torch.bool),
                torch.ones(2, 3, 6, dtype=torch.bool), torch.ones(1, 3, 3, 6, dtype=torch.bool)):
        with pytest.raises(ValueError, match="block_map shape"):
            sa.sageattn_block_sparse(q, k, k, bad)
    with pytest.raises(ValueError, match="block_map shape"):  # the map's geometry follows the layout's sequence axis
        sa.sageattn_block_sparse(q.transpose(1, 2), k.transpose(1, 2), k.transpose(1, 2), good)
    with pytest.raises(ValueError, match="pv"):
        sa.sageattn_block_sparse(q, k, k, good, pv="auto")
    with pytest.raises(ValueError, match="qk_quant_gran"):
        sa.sageattn_block_sparse(q, k, k, good, qk_quant_gran="per_block")
    with pytest.raises(ValueError, match="is on"):
        sa.sageattn_block_sparse(q, k, k, good.to("meta"))
    plan = sa.BlockSparsePlan(torch.zeros(72, dtype=torch.int32), 1, 2, 300, 400)
    with pytest.raises(ValueError, match="plan was made for"):
        sa.sageattn_block_sparse(q, k, k, plan)
    with pytest.raises(ValueError, match="contiguous int32"):  # lists of another size than this shape's
        sa.sageattn_block_sparse(q, k, k, sa.BlockSparsePlan(torch.zeros(80, dtype=torch.int32), 1, 2, 300, 333))
    with pytest.raises(TypeError):  # unknown keywords are not swallowed
        sa.sageattn_block_sparse(q, k, k, good, attn_mask=None)
    with pytest.raises(TypeError, match="dtype"):  # the map op takes maps only; plans go through attn_block_sparse_plan
        torch.ops.sageattention_amd.attn_block_sparse(q, k, k, torch.zeros(72, dtype=torch.int32), "HND", 0.125, "fp16",
                                                      "per_thread")
    with pytest.raises(ValueError, match="plan was made for"):
        torch.ops.sageattention_amd.attn_block_sparse_plan(q, k, k, torch.zeros(72, dtype=torch.int32), [1, 2, 300, 400],
                                                           "HND", 0.125, "fp16", "per_thread")
    with pytest.raises(ValueError, match="GPU"):
        sa.block_sparse_plan(good, 300, 333)
    with pytest.raises(AssertionError, match="cuda"):  # as every operator of the package on CPU tensors
        sa.sageattn_block_sparse(q, k, k, good)


# ---- 5. the torch.library op ------------------------------------------------------------------------------------------------
def test_op_schema_and_fake_shapes():
    import sageattention_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    s = str(torch.ops.sageattention_amd.attn_block_sparse.default._schema)
    assert "Tensor q, Tensor k, Tensor v, Tensor block_map, str tensor_layout, float sm_scale, str pv, str qk_quant_gran" in s
    with FakeTensorMode():
        for layout, shp, kshp in (("HND", (2, 8, 300, 96), (2, 4, 333, 96)), ("NHD", (2, 300, 8, 96), (2, 333, 4, 96))):
            q = torch.empty(shp, dtype=torch.bfloat16, device="cuda")
            k = torch.empty(kshp, dtype=torch.bfloat16, device="cuda")
            bm = torch.empty((2, 8, 3, 6), dtype=torch.bool, device="cuda")
            o = ops.sageattn_block_sparse_compilable(q, k, k, bm, tensor_layout=layout, pv="fp8")
            assert o.shape == q.shape and o.dtype == q.dtype and o.device == q.device and o.is_contiguous()
    assert "[] plan_shape, str tensor_layout" in str(torch.ops.sageattention_amd.attn_block_sparse_plan.default._schema)
    o = torch.ops.sageattention_amd.attn_block_sparse(torch.empty(1, 2, 130, 64, device="meta", dtype=torch.float16),
                                                      torch.empty(1, 2, 70, 64, device="meta", dtype=torch.float16),
                                                      torch.empty(1, 2, 70, 64, device="meta", dtype=torch.float16),
                                                      torch.empty(1, 2, 2, 2, device="meta", dtype=torch.bool), "HND", 0.125,
                                                      "fp16", "per_thread")
    assert o.shape == (1, 2, 130, 64) and o.device.type == "meta"
    with pytest.raises(ValueError):
        ops.sageattn_block_sparse_compilable(torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64),
                                             torch.ones(1, 1, 1, 1, dtype=torch.bool), tensor_layout="BHSD")
