"""The P.V skip of block-sparse attention without a GPU: the inputs of tests/test_pvskip_gpu.py are firm, the torch
restatement of the rule (tests/pvskip_util.py) is pinned by a hand-counted case, the Python keywords and the four C entry
points refuse what they must, and the new custom ops exist beside the unchanged old ones."""
import math

import pytest
import torch

import pvskip_util as U

LAZY16 = 6 * math.log(2.0)  # the larger of the two lazy-rescale lags (FP16 / BF16 PV); FP8 PV: 3 ln 2


def _gpu_configs():
    import test_pvskip_gpu as G
    return sorted({(D, gran, dtype) for D, _, gran, dtype in G.FIRM_CASES} | {(64, "per_thread", torch.float16),
                                                                            (128, "per_warp", torch.float16)}, key=str)


@pytest.mark.parametrize("cfg", _gpu_configs(), ids=lambda c: "-".join(str(x).replace("torch.", "") for x in c))
def test_gpu_inputs_are_firm(cfg):
    """every skipping gap >= pvthreshd + 6 ln 2 + 1 and every other gap <= pvthreshd - 1: the kernel's lagging reference
    maximum and its fp32 arithmetic cannot decide differently from the fp64 restatement"""
    import test_pvskip_gpu as G
    D, gran, dtype = cfg
    _, _, _, bm, logits, skipped, counts, min_skip, max_keep = U.firm_case(D, gran, dtype, G.THR)
    assert min_skip >= G.THR + LAZY16 + 1, min_skip
    assert max_keep <= G.THR - 1, max_keep
    # what the inputs are meant to hit
    assert any(p and p + 1 in s for s in skipped.values() for p in s), "two skips in a row"
    full = [key for key in skipped if bm[key[0], key[1], key[2]].all()]
    assert any({8, 9} & skipped[key] == {9} for key in full) and any({8, 9} & skipped[key] == {8} for key in full), \
        "a skip on the last (ragged) tile and on the tile before it"
    assert counts[0, 0, 0].tolist() == [6, 4, 6, 2], "waves of one workgroup decide differently; the mixed wave skips least"
    assert counts[:, :, 1, 3].sum() == 0 and counts[0, 1, 1, 2] > 0, "a wave without rows < M; a wave with 8 of them"
    # the variants of the per-head and the empty q-block tests
    _, c2, lo, hi = U.restate(logits, bm, [math.inf, G.THR])
    assert c2[:, 0].sum() == 0 and torch.equal(c2[:, 1], counts[:, 1]) and lo >= G.THR + LAZY16 + 1 and hi <= G.THR - 1
    bm2 = bm.clone()
    bm2[0, 1, 0] = False
    bm2[1, 0, 1] = False
    _, c3, lo, hi = U.restate(logits, bm2, G.THR)
    assert c3[0, 1, 0].sum() == 0 and c3[1, 0, 1].sum() == 0 and lo >= G.THR + LAZY16 + 1 and hi <= G.THR - 1


def test_first_tile_negligible_is_still_computed():
    """head 1 (axis 1) starts on a tile 30 below its best: position 0 is never skipped, and the tile at position 1 lifts the
    maximum instead of being compared against the negligible one"""
    _, _, _, bm, logits, skipped, _, _, _ = U.firm_case(64, "per_thread", torch.float16, 16.0)
    assert bm[0, 1, 0, :3].all()  # list positions 0..2 are tiles 0..2
    t0 = logits[0, 1, :32, :64].amax(-1)
    t1 = logits[0, 1, :32, 64:128].amax(-1)
    assert (t1 - t0).min() > 25
    assert 0 not in skipped[(0, 1, 0, 0)] and 1 not in skipped[(0, 1, 0, 0)] and 2 in skipped[(0, 1, 0, 0)]


def test_restatement_on_a_hand_counted_case():
    """M = 40 (wave 0 full, wave 1 with 8 rows, waves 2 and 3 without rows), N = 150 (tiles of 64, 64 and 22 keys), thr = 5.
    Tile 0 is 0 everywhere.  Tile 1 is -10, except -3 in row 5.  Tile 2 is -10, except -1 in row 33 at the last key.
      wave 0: pos 1 kept (row 5: gap 3 < 5), pos 2 skipped (gap 10)                    -> {2}
      wave 1: pos 1 skipped (gap 10), pos 2 kept (row 33: gap 1)                       -> {1}
    smallest skipping gap 10, largest kept gap 3."""
    lg = torch.zeros(1, 1, 40, 150, dtype=torch.float64)
    lg[..., 64:] = -10.0
    lg[0, 0, 5, 100] = -3.0
    lg[0, 0, 33, 149] = -1.0
    bm = torch.ones(1, 1, 1, 3, dtype=torch.bool)
    skipped, counts, lo, hi = U.restate(lg, bm, 5.0)
    assert skipped == {(0, 0, 0, 0): {2}, (0, 0, 0, 1): {1}, (0, 0, 0, 2): set(), (0, 0, 0, 3): set()}
    assert counts.flatten().tolist() == [1, 1, 0, 0] and lo == 10.0 and hi == 3.0
    # a list without tile 0: the first tile of the LIST is never skipped, however small, and later gaps are taken against it
    skipped, counts, lo, hi = U.restate(lg - 100.0 * (torch.arange(150) >= 128), torch.tensor([[[[False, True, True]]]]), 5.0)
    assert skipped[(0, 0, 0, 0)] == {1} and skipped[(0, 0, 0, 1)] == {1} and counts.flatten().tolist() == [1, 1, 0, 0]
    # thresholds that disable the skip
    for off in (0.0, -1.0, math.inf, math.nan):
        assert U.restate(lg, bm, off)[1].sum() == 0
    # switching a wave's skipped tiles off in the map
    assert U.map_without(bm, U.restate(lg, bm, 5.0)[0], 0).flatten().tolist() == [True, True, False]
    assert U.wave_rows(200, 2).nonzero().flatten().tolist() == list(range(64, 96)) + list(range(192, 200))


def test_loose_inputs_do_skip():
    """the inputs of the error-bound test: some wave-tile is certainly skipped under either P.V type, and they are not firm"""
    import test_pvskip_gpu  # noqa: F401  (the cases of its bound test)
    for D, pv, gran in ((64, "fp16", "per_thread"), (128, "fp8", "per_warp"), (64, "fp8", "per_thread"),
                        (128, "fp16", "per_thread")):
        _, _, _, bm, logits = U.loose_case(D, gran, torch.float16)
        _, certain, _, _ = U.restate(logits, bm, 20.0 + U.LAZY[pv])
        _, upper, lo, hi = U.restate(logits, bm, 20.0)
        assert certain.sum() > 0 and (upper >= certain).all()
        assert lo < 20.0 + U.LAZY[pv] + 1 or hi > 20.0 - 1


def test_python_keywords_are_checked_before_any_tensor_is_touched():
    from sageattention_amd import core, ops
    x = object()  # not a tensor: any access would raise something else
    for fn in (core.sageattn_block_sparse, ops.sageattn_block_sparse_compilable):
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="pvthreshd"):
                fn(x, x, x, x, pvthreshd=bad)
        with pytest.raises(ValueError, match="return_skipped"):
            fn(x, x, x, x, return_skipped=True)
    for fn in (core.sageattn_sparge, ops.sageattn_sparge_compilable):
        for bad in (0.0, -2.5, float("nan")):
            with pytest.raises(ValueError, match="pvthreshd"):
                fn(x, x, x, pvthreshd=bad)
        with pytest.raises(ValueError, match="return_skipped"):
            fn(x, x, x, return_skipped=True)
    with pytest.raises(ValueError, match=r"pvthreshd must be a float or a tensor of shape \[Hq=4\]"):
        core._pvskip_tensors(torch.ones(3), True, 1, 4, 128, "cpu")
    thr, sk = core._pvskip_tensors(2.0, True, 2, 4, 200, "cpu")
    assert thr.tolist() == [2.0] * 4 and thr.dtype == torch.float32 and tuple(sk.shape) == (2, 4, 2, 4) and sk.dtype == torch.int32
    assert core._pvskip_tensors(None, False, 2, 4, 200, "cpu") == (None, None)
    assert core._pvskip_tensors(torch.tensor([1.0, float("inf"), -1.0, float("nan")]), False, 1, 4, 64, "cpu")[1] is None


OLD_SCHEMAS = {
    "attn": "(Tensor q, Tensor k, Tensor v, str tensor_layout, bool is_causal, float sm_scale, str pv, str qk_quant_gran) -> Tensor",
    "attn_lse": "(Tensor q, Tensor k, Tensor v, str tensor_layout, bool is_causal, float sm_scale, str pv, str qk_quant_gran) "
                "-> (Tensor, Tensor)",
    "attn_block_sparse": "(Tensor q, Tensor k, Tensor v, Tensor block_map, str tensor_layout, float sm_scale, str pv, "
                         "str qk_quant_gran) -> Tensor",
    "attn_block_sparse_plan": "(Tensor q, Tensor k, Tensor v, Tensor block_lists, SymInt[] plan_shape, str tensor_layout, "
                              "float sm_scale, str pv, str qk_quant_gran) -> Tensor",
    "attn_sparge": "(Tensor q, Tensor k, Tensor v, Tensor simthreshd1, Tensor cdfthreshd, str tensor_layout, float sm_scale, "
                   "str pv, str qk_quant_gran) -> Tensor",
    "attn_sparge_lse": "(Tensor q, Tensor k, Tensor v, Tensor simthreshd1, Tensor cdfthreshd, str tensor_layout, "
                       "float sm_scale, str pv, str qk_quant_gran) -> (Tensor, Tensor)",
    "attn_sparge_select": "(Tensor q, Tensor k, Tensor v, Tensor simthreshd1, Tensor rule_param, str rule, SymInt keep_first, "
                          "SymInt keep_last, str tensor_layout, float sm_scale, str pv, str qk_quant_gran) -> Tensor",
    "attn_sparge_select_lse": "(Tensor q, Tensor k, Tensor v, Tensor simthreshd1, Tensor rule_param, str rule, "
                              "SymInt keep_first, SymInt keep_last, str tensor_layout, float sm_scale, str pv, "
                              "str qk_quant_gran) -> (Tensor, Tensor)",
}
NEW_SCHEMAS = {
    "attn_block_sparse_pv": "(Tensor q, Tensor k, Tensor v, Tensor block_map, Tensor pvthreshd, str tensor_layout, "
                            "float sm_scale, str pv, str qk_quant_gran) -> (Tensor, Tensor)",
    "attn_block_sparse_plan_pv": "(Tensor q, Tensor k, Tensor v, Tensor block_lists, SymInt[] plan_shape, Tensor pvthreshd, "
                                 "str tensor_layout, float sm_scale, str pv, str qk_quant_gran) -> (Tensor, Tensor)",
    "attn_sparge_pv": "(Tensor q, Tensor k, Tensor v, Tensor simthreshd1, Tensor rule_param, str rule, SymInt keep_first, "
                      "SymInt keep_last, Tensor pvthreshd, str tensor_layout, float sm_scale, str pv, str qk_quant_gran) "
                      "-> (Tensor, Tensor)",
    "attn_sparge_pv_lse": "(Tensor q, Tensor k, Tensor v, Tensor simthreshd1, Tensor rule_param, str rule, SymInt keep_first, "
                          "SymInt keep_last, Tensor pvthreshd, str tensor_layout, float sm_scale, str pv, str qk_quant_gran) "
                          "-> (Tensor, Tensor, Tensor)",
}


def test_new_op_schemas_exist_and_the_old_ones_are_unchanged():
    import sageattention_amd.ops  # noqa: F401
    for name, sig in {**OLD_SCHEMAS, **NEW_SCHEMAS}.items():
        assert str(getattr(torch.ops.sageattention_amd, name).default._schema) == f"sageattention_amd::{name}{sig}"


def test_fake_implementations_describe_the_counters():
    """shapes and dtypes under meta tensors: what torch.compile traces"""
    import sageattention_amd.ops  # noqa: F401
    q = torch.empty(2, 4, 200, 64, dtype=torch.float16, device="meta")
    kv = torch.empty(2, 2, 616, 64, dtype=torch.float16, device="meta")
    thr = torch.empty(4, device="meta")
    bm = torch.empty(2, 4, 2, 10, dtype=torch.bool, device="meta")
    o, sk = torch.ops.sageattention_amd.attn_block_sparse_pv(q, kv, kv, bm, thr, "HND", 0.125, "fp16", "per_thread")
    assert o.shape == q.shape and tuple(sk.shape) == (2, 4, 2, 4) and sk.dtype == torch.int32
    o, lse, sk = torch.ops.sageattention_amd.attn_sparge_pv_lse(q, kv, kv, thr, thr, "cdf", 0, 0, thr, "HND", 0.125, "fp8",
                                                                "per_warp")
    assert tuple(lse.shape) == (2, 4, 200) and lse.dtype == torch.float32 and tuple(sk.shape) == (2, 4, 2, 4)
    qn = q.transpose(1, 2)  # NHD: [B, M, H, D]
    o, sk = torch.ops.sageattention_amd.attn_sparge_pv(qn, kv, kv, thr, thr, "topk", 1, 0, thr, "NHD", 0.125, "fp16", "per_thread")
    assert tuple(o.shape) == (2, 200, 4, 64) and tuple(sk.shape) == (2, 4, 2, 4)


# ---- the four entry points check their arguments before any launch (fake device addresses: only where no GPU is visible,
#      where every launch attempt returns SAGE_ERR_LAUNCH = -5, as tests/test_cabi_symbols.py does it)
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")
FAKE, ODD4 = 1 << 20, (1 << 20) + 2

_PV_PARAMS = {
    "sage_attn_qk_int8_pv_f16_blocksparse_pvskip":
        "q k v vdt o odt qs ks vm lse B Hq Hk M N D causal gran blkq warpq sm lm1 lists lbytes thr skipped stream",
    "sage_attn_qk_int8_pv_f8_blocksparse_pvskip":
        "q k v o odt qs ks vs vm lse B Hq Hk M N D causal gran blkq warpq sm lm1 lists lbytes thr skipped stream",
    "sage_attn_fusedq_pv_f16_blocksparse_pvskip":
        "q qdt k v vdt o odt ks km vm lse B Hq Hk M N D causal gran warpq sm lists lbytes thr skipped stream",
    "sage_attn_fusedq_pv_f8_blocksparse_pvskip":
        "q qdt k v o odt ks km vs vm lse B Hq Hk M N D causal gran warpq sm lists lbytes thr skipped stream",
}


def _call(fn, **change):
    from sageattention_amd import _build, _lib as L
    _build.build()
    t = L.SageTensor(FAKE, 1 << 16, 1 << 12, 64)
    args = dict(q=t, k=t, v=t, vdt=0, o=t, odt=0, qdt=0, qs=FAKE, ks=FAKE, vs=FAKE, km=FAKE, vm=None, lse=None, B=1, Hq=2, Hk=1,
                M=64, N=64, D=64, causal=0, gran=3, blkq=128, warpq=32, sm=0.125, lm1=0, lists=FAKE, lbytes=1 << 20, thr=FAKE,
                skipped=FAKE, stream=None)
    args.update(change)
    return getattr(L.lib(), fn)(*[args[n] for n in _PV_PARAMS[fn].split()])


@no_gpu
@pytest.mark.parametrize("fn", sorted(_PV_PARAMS))
def test_entry_points_check_before_any_launch(fn):
    assert _call(fn) == -5                       # the control: a valid call reaches a launch
    assert _call(fn, skipped=None) == -5         # the counters are optional
    assert _call(fn, thr=None) == -1             # SAGE_ERR_INVALID_ARGUMENT
    assert _call(fn, thr=ODD4) == -1
    assert _call(fn, skipped=ODD4) == -1
    assert _call(fn, lists=None) == -1           # as the twin
    assert _call(fn, causal=1) == -3             # SAGE_ERR_UNSUPPORTED, as the twin
    assert _call(fn, vm=FAKE) == -3
    assert _call(fn, D=96) == -2
    # the argument statuses come before the unsupported combinations, as the twin orders its list check
    assert _call(fn, thr=None, causal=1) == -1


def test_abi_version_and_binding():
    from sageattention_amd import _build, _lib as L
    _build.build()
    assert L.lib().sage_abi_version() == 3
    for fn in _PV_PARAMS:
        assert len(L.SIGNATURES[fn][1]) == len(_PV_PARAMS[fn].split())
        twin = fn[:-len("_pvskip")]
        assert L.SIGNATURES[fn][1][:len(L.SIGNATURES[twin][1]) - 1] == L.SIGNATURES[twin][1][:-1]
