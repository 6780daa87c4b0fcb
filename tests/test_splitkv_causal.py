"""Causal split-KV attention (``sageattn_splitkv_causal``, ``sage_attn_fusedq_pv_{f16,f8}_splitkv_causal``) without a GPU:
the bookkeeping of the rule (which workgroups run, how many slots the merge reads), the Python refusals and the ``q_fold``
checks, the C status table of the two entry points, the torch.library ops, and the soundness and the teeth of the oracle of
tests/splitkv_causal_util.py.  What the kernels compute: test_splitkv_causal_gpu.py."""
import pytest
import torch

import constructed_cases as C
import splitkv_causal_util as CU


# ---- 1. the rule's bookkeeping ---------------------------------------------------------------------------------------------
def test_qblock_counts_are_the_splits_that_keep_a_key():
    """over a sweep of (len, T, g, S): the count of q-block qb equals the number of splits in which some row of the q-block
    keeps a key, those are the FIRST splits and exactly the workgroups that run, and the counts are monotone in qb"""
    seen_zero = seen_partial = 0
    for length in (0, 1, 63, 64, 65, 100, 257, 456, 512, 1000):
        for T in (1, 4, 30, 75, 150, 300, 1100):
            for g in (1, 2, 5, 8):
                M = T * g
                ok = CU.allowed_keys(length, M, g)
                assert ok.shape == (M, length)
                # row r: keys 0 .. r // g + len - T, clipped to [0, len)
                for r in (0, M // 2, M - 1):
                    want = max(0, min(length, r // g + length - T + 1))
                    assert int(ok[r].sum()) == want and bool(ok[r, :want].all()), (length, T, g, r)
                nqb = (M + 127) // 128
                for S in (1, 2, 3, 5, 8, 16):
                    counts = []
                    for qb in range(nqb):
                        rows = ok[128 * qb:128 * qb + 128]
                        keeps = []
                        for s in range(S):
                            t0, t1 = CU.split_range(length, S, s)
                            keeps.append(bool(rows[:, 64 * t0:64 * t1].any()))
                        cnt = CU.qblock_count(length, M, g, S, qb)
                        assert keeps == [s < cnt for s in range(S)], (length, T, g, S, qb, keeps, cnt)
                        assert keeps == [CU.runs(length, M, g, S, qb, s) and CU.split_range(length, S, s)[0] <
                                         CU.split_range(length, S, s)[1] for s in range(S)], (length, T, g, S, qb)
                        counts.append(cnt)
                    assert counts == sorted(counts), (length, T, g, S, counts)
                    seen_zero += counts[0] == 0 and length > 0
                    seen_partial += 0 < counts[0] < counts[-1]
    assert seen_zero and seen_partial  # q-blocks without any key in a batch that has keys; counts that differ within a head


def test_anchor_coincides_with_top_left():
    """len = T, g = 1: off = 0, the band is the top-left triangle"""
    ok = CU.allowed_keys(70, 70, 1)
    assert torch.equal(ok, torch.ones(70, 70).tril().bool())
    assert bool(CU.allowed_keys(1000, 1, 1).all())  # one token sees every valid key


# ---- 2. Python refusals, raised before any device call -----------------------------------------------------------------------
def test_python_refusals():
    import sageattention_amd as sa
    from sageattention_amd import core
    import sageattention
    f = sa.sageattn_splitkv_causal
    assert "sageattn_splitkv_causal" in sa.__all__ and "sageattn_splitkv_causal" in core.__all__ and f is core.sageattn_splitkv_causal
    assert sageattention.sageattn_splitkv_causal is f and sageattention.core.sageattn_splitkv_causal is f
    q = torch.zeros(2, 4, 70, 64, dtype=torch.float16)
    k = torch.zeros(2, 2, 1000, 64, dtype=torch.float16)
    lens = torch.tensor([1000, 7], dtype=torch.int32)
    for kw in (dict(is_causal=False), dict(attn_mask=torch.ones(70, 1000, dtype=torch.bool)), dict(smooth_k=False),
               dict(smooth_v=True), dict(block_map=torch.ones(1, 1, 1, 16, dtype=torch.bool)), dict(plan=object()),
               dict(cu_seqlens_q=torch.zeros(3, dtype=torch.int32)), dict(cu_seqlens_k=torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError, match="does not take"):
            f(q, k, k, num_splits=2, **kw)
    with pytest.raises(TypeError, match="unexpected keyword"):
        f(q, k, k, num_splits=2, window=3)
    with pytest.raises(TypeError, match="int32"):
        f(q, k, k, lens.long(), 2)
    with pytest.raises(ValueError, match="kv_lens shape"):
        f(q, k, k, torch.zeros(3, dtype=torch.int32), 2)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="num_splits"):
            f(q, k, k, num_splits=bad)
    with pytest.raises(TypeError, match="num_splits"):
        f(q, k, k, num_splits=2.0)
    for bad in (0, -2, 3, 4, 140):  # 70 rows: 3 and 4 do not divide them, 140 is more than there are
        with pytest.raises(ValueError, match="q_fold"):
            f(q, k, k, num_splits=2, q_fold=bad)
    for bad in (True, 2.0, None, "2"):
        with pytest.raises(TypeError, match="q_fold"):
            f(q, k, k, num_splits=2, q_fold=bad)
    with pytest.raises(ValueError, match="pv"):
        f(q, k, k, num_splits=2, pv="int8")
    with pytest.raises(ValueError, match="qk_quant_gran"):
        f(q, k, k, num_splits=2, qk_quant_gran="per_block")
    with pytest.raises(ValueError, match="layout"):
        f(q, k, k, num_splits=2, tensor_layout="BHSD")
    with pytest.raises(ValueError, match="one shape"):
        f(q, k, k[..., :32], lens, 2, pv="fp8")
    for fold in (1, 2, 70):  # valid folds, is_causal=True accepted, num_splits 1 valid: the CPU tensors are what stops the call
        with pytest.raises(AssertionError, match="cuda"):
            f(q, k, k, lens, 1, fold, is_causal=True)
    # the non-causal operator is untouched: it still refuses is_causal by name
    with pytest.raises(ValueError, match="does not take is_causal=True"):
        sa.sageattn_splitkv(q, k, k, num_splits=2, is_causal=True)


# ---- 3. the C status table ---------------------------------------------------------------------------------------------------
# Fake device addresses, as in tests/test_splitkv.py: only where no GPU is visible; a launch attempt returns SAGE_ERR_LAUNCH (-5)
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")

FAKE = 1 << 20
_PARAMS = {
    "sage_attn_fusedq_pv_f16_splitkv_causal":
        "q qdt k v vdt o odt ks km vm lse B Hq Hk M N D gran warpq sm lens S fold ws wsb stream",
    "sage_attn_fusedq_pv_f8_splitkv_causal":
        "q qdt k v o odt ks km vs vm lse B Hq Hk M N D gran warpq sm lens S fold ws wsb stream",
}
_B, _HQ, _M, _D, _S = 2, 2, 200, 64, 5
_NEED = _S * _B * _HQ * _M * (_D + 1) * 4


def _call(fn, **change):
    from sageattention_amd import _lib as L
    t = L.SageTensor(FAKE, 1 << 16, 1 << 12, 64)
    args = dict(q=t, k=t, v=t, o=t, vdt=0, odt=0, qdt=0, ks=FAKE, vs=FAKE, vm=None, km=FAKE, lse=None, B=_B, Hq=_HQ, Hk=1, M=_M,
                N=333, D=_D, gran=3, warpq=32, sm=0.125, lens=FAKE, S=_S, fold=1, ws=FAKE, wsb=_NEED, stream=None)
    args.update(change)
    return getattr(L.lib(), fn)(*[args[n] for n in _PARAMS[fn].split()])


@no_gpu
def test_valid_calls_reach_a_launch():
    for fn in _PARAMS:
        assert _call(fn) == -5
        assert _call(fn, lens=None, lse=FAKE, S=1, wsb=_B * _HQ * _M * (_D + 1) * 4, qdt=1, odt=1) == -5  # one split is valid
        assert _call(fn, S=16, wsb=16 * _B * _HQ * _M * (_D + 1) * 4, gran=2, fold=8) == -5
        for fold in (2, 5, 200):
            assert _call(fn, fold=fold) == -5
        assert _call(fn, N=7, M=200, fold=1) == -5  # a chunk longer than the cache: valid


@no_gpu
def test_status_table():
    """Each argument made invalid on its own returns its argument status: nothing was launched (a launch returns -5 here).
    The statuses of the non-causal entry points (tests/test_splitkv.py), and q_fold < 1 or not a divisor of M: -1."""
    cases = []
    for fn in _PARAMS:
        cases += [(fn, dict(fold=0), -1), (fn, dict(fold=-1), -1), (fn, dict(fold=3), -1), (fn, dict(fold=400), -1),
                  (fn, dict(S=0), -1), (fn, dict(S=17), -1), (fn, dict(S=-1), -1), (fn, dict(ws=None), -1),
                  (fn, dict(ws=FAKE + 8), -1), (fn, dict(wsb=_NEED - 1), -1), (fn, dict(wsb=0), -1), (fn, dict(lens=FAKE + 2), -1),
                  (fn, dict(gran=1), -3), (fn, dict(km=None), -3), (fn, dict(km=FAKE + 8), -3), (fn, dict(vm=FAKE), -3),
                  (fn, dict(N=1 << 25), -4), (fn, dict(D=96), -2), (fn, dict(N=0), -1), (fn, dict(B=0), -1), (fn, dict(M=0), -1),
                  (fn, dict(ks=None), -1), (fn, dict(sm=0.0), -1), (fn, dict(Hk=3), -1), (fn, dict(qdt=2), -1),
                  (fn, dict(odt=2), -1), (fn, dict(gran=0), -1), (fn, dict(q=None), -1), (fn, dict(o=None), -1)]
    cases += [("sage_attn_fusedq_pv_f8_splitkv_causal", dict(vs=None), -1),
              ("sage_attn_fusedq_pv_f16_splitkv_causal", dict(vdt=2), -1)]
    wrong = [(fn, sorted(c), st, got) for fn, c, st in cases if (got := _call(fn, **c)) != st]
    assert not wrong, wrong


# ---- 4. the torch.library ops ----------------------------------------------------------------------------------------------
def test_op_schemas_and_fake_shapes():
    import sageattention_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    want = ("Tensor q, Tensor k, Tensor v, Tensor? kv_lens, SymInt num_splits, SymInt q_fold, str tensor_layout, "
            "float sm_scale, str pv, str qk_quant_gran")
    s, s_lse = (str(getattr(torch.ops.sageattention_amd, n).default._schema)
                for n in ("attn_splitkv_causal", "attn_splitkv_causal_lse"))
    assert want in s and s.endswith("-> Tensor")
    assert want in s_lse and s_lse.endswith("-> (Tensor, Tensor)")
    assert "sageattn_splitkv_causal_compilable" in ops.__all__
    f = ops.sageattn_splitkv_causal_compilable
    with FakeTensorMode():
        for layout, shp, kshp in (("HND", (3, 8, 70, 72), (3, 4, 1000, 72)), ("NHD", (3, 70, 8, 72), (3, 1000, 4, 72))):
            q = torch.empty(shp, dtype=torch.bfloat16, device="cuda")
            k = torch.empty(kshp, dtype=torch.bfloat16, device="cuda")
            lens = torch.empty((3,), dtype=torch.int32, device="cuda")
            o = f(q, k, k, lens, 4, 2, tensor_layout=layout, pv="fp8")
            assert o.shape == q.shape and o.dtype == q.dtype and o.device == q.device and o.is_contiguous()
            o, lse = f(q, k, k, tensor_layout=layout, return_lse=True)
            assert o.shape == q.shape and lse.shape == (3, 8, 70) and lse.dtype == torch.float32
    z = torch.zeros(1, 1, 4, 64)
    with pytest.raises(ValueError, match="layout"):
        f(z, z, z, tensor_layout="BHSD")
    with pytest.raises(ValueError, match="num_splits"):
        f(z, z, z, num_splits=17)


# ---- 5. the oracle is sound and has teeth ------------------------------------------------------------------------------------
# Small enough for the CPU: head_dim 64, one ramp (LSEs of the splits far apart), the scale ladder (neighbouring tiles with
# different scales) and a one-hot case whose hot key is the LAST valid one at length 257 (the key only the last token's rows
# may see).  N = 512 and 456 (ragged), lengths N, 257 (off = 107: the split edges cut through a wave's diagonal span) and 100
# (< T: rows without keys), folds 1, 2, 5, S = 1, 3, 8.
def _teeth_cases():
    yield "ramp", C.ramp(64, 512, False, "per_warp", "40", "ascending", anchor=True)
    yield "ladder", C.anchor(C.scale_ladder(64, 456, False, "per_thread"))
    yield "hot256", C.anchor(C.one_hot(64, 512, False, "per_warp", 256))


@pytest.fixture(scope="module")
def restated():
    """{mistake or None: largest ratio over the sweep} and, for the correct restatement, every case's ratios"""
    worst = {m: 0.0 for m in (None,) + CU.MISTAKES}
    bad = []
    for label, c in _teeth_cases():
        qkm = C.split_qkm(c, C.split_km(64, True))
        for length in (c["N"], 257, 100):
            for g in (1, 2, 5):
                for S in (1, 3, 8):
                    for m in worst:
                        o, lse = CU.restate64(c, "fp16", length, g, S, m, qkm)
                        ro, rl, empty_ok = CU.check(c, "fp16", length, g, S, o, lse, qkm, torch.float16)
                        r = max(ro, rl) if empty_ok else float("inf")
                        worst[m] = max(worst[m], r)
                        if m is None and not r <= 1.0:
                            bad.append((label, length, g, S, ro, rl, empty_ok))
    return worst, bad


def test_oracle_is_sound(restated):
    """the float64 restatement of the kernels as written -- split-local limits, per-q-block counts, -inf slots dropped -- stays
    within the bound on every element of every case (it differs from the reference by float64 rounding only)"""
    worst, bad = restated
    assert not bad, bad[:10]
    assert worst[None] < 1e-3, worst[None]


@pytest.mark.parametrize("mistake", CU.MISTAKES)
def test_oracle_has_teeth(restated, mistake):
    """each named mistake exceeds the bound somewhere in the sweep"""
    worst, _ = restated
    assert worst[mistake] > 1.0, (mistake, worst[mistake])
