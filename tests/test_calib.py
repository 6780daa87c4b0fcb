"""Calibration of the block-map predictor without a GPU: the fp64 restatement (tests/calib_util.py) has the properties the
definition promises, the bindings and the Python keywords are what the interface declares, the two C entry points refuse
what they must before any launch, and the tolerance of tests/test_calib_gpu.py is tight enough to see two planted mistakes."""
import ctypes
import inspect
import math

import pytest
import torch

import calib_util as C
import pvskip_util as PU
import sparge_util as SU


def _logits(B, H, M, N, seed, spread=4.0):
    return spread * torch.randn(B, H, M, N, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(200, 616), (1, 40), (129, 64), (128, 64)])
def test_rows_of_the_tile_mass_sum_to_one(M, N):
    mass = C.tile_mass(_logits(2, 3, M, N, 1), M, N)
    assert tuple(mass.shape) == (2, 3, (M + 127) // 128, (N + 63) // 64)
    assert (mass >= 0).all() and ((mass.sum(-1) - 1).abs() <= 1e-12).all()


def test_ragged_tile_and_ragged_q_block_are_weighted_by_what_is_valid():
    M, N = 200, 616
    flat = C.tile_mass(torch.zeros(1, 1, M, N, dtype=torch.float64), M, N)  # uniform attention
    keys = torch.tensor([64.0] * 9 + [40.0], dtype=torch.float64) / N
    assert ((flat - keys).abs() <= 1e-15).all()  # both q-blocks alike: 128 and 72 valid rows
    # every row of the second q-block looks at key 615 alone: its last tile holds all the mass, whatever c_i is
    lg = torch.zeros(1, 1, M, N, dtype=torch.float64)
    lg[0, 0, 128:, 615] = 200.0
    mass = C.tile_mass(lg, M, N)
    assert abs(float(mass[0, 0, 1, 9]) - 1.0) <= 1e-12 and float(mass[0, 0, 1, :9].sum()) <= 1e-12
    assert ((mass[0, 0, 0] - keys).abs() <= 1e-15).all()
    # ... and the planted mistakes get exactly these two wrong
    assert abs(float(C.tile_mass_weights_128(lg, M, N)[0, 0, 1, 9]) - 72 / 128) <= 1e-12
    assert abs(float(C.tile_mass_counts_padding(torch.zeros(1, 1, M, N, dtype=torch.float64), M, N)[0, 0, 0, 9]) - 64 / 640) <= 1e-15


def test_recall_and_head_recall():
    M, N = 200, 616
    mass = C.tile_mass(_logits(2, 2, M, N, 2), M, N)
    bm = torch.zeros(2, 2, 2, 10, dtype=torch.bool)
    bm[..., ::3] = True
    bm[1, 1, 0] = False
    rec, kept = C.recall(bm, mass)
    assert float(rec[1, 1, 0]) == 0.0 and int(kept[1, 1, 0]) == 0 and int(kept[0, 0, 0]) == 4
    assert torch.allclose(rec[0, 0, 1], mass[0, 0, 1, ::3].sum())
    full, _ = C.recall(torch.ones(1, 1, 2, 10, dtype=torch.bool), mass)
    assert ((C.head_recall(full, M, "mean") - 1).abs() <= 1e-12).all() and ((C.head_recall(full, M, "min") - 1).abs() <= 1e-12).all()
    want = (rec[:, :, 0] * 128 + rec[:, :, 1] * 72).sum(0) / (2 * M)
    assert torch.allclose(C.head_recall(rec, M, "mean"), want)
    assert torch.equal(C.head_recall(rec, M, "min"), rec.amin((0, 2)))


@pytest.mark.parametrize("reduce", ["mean", "min"])
def test_brute_force_tune_is_monotone(reduce):
    """on the clustered inputs, with the fp64 restatement of the predictor's rule as the map: head recall never falls as
    cdfthreshd grows, and param / recall / recall_below bracket the target"""
    steps, target = 4, 0.95
    r = SU.ref("c1")
    mass = C.tile_mass(PU.scaled_logits(r.q, r.k, "per_thread"), r.M, r.N)

    def head_recall_at(g):
        return C.head_recall(C.recall(r.map(g / 2 ** steps), mass)[0], r.M, reduce)
    param, met, rec, below, table = C.tune(head_recall_at, steps, target)
    assert (table[1:] >= table[:-1] - 1e-15).all()
    assert met.all() and ((table[-1] - 1).abs() <= 1e-12).all()  # cdfthreshd = 1 keeps every tile
    assert (rec >= target).all() and (below < target).all()
    for h in range(r.Hq):
        g = int(round(float(param[h]) * 2 ** steps))
        assert float(table[g - 1, h]) == float(rec[h])
        assert float(below[h]) == (float(table[g - 2, h]) if g > 1 else -math.inf)
        assert (table[:g - 1, h] < target).all()
    # a target nothing meets: param 1.0, met False
    param, met, rec, below, _ = C.tune(lambda g: torch.full((2,), 0.5 * g / 16, dtype=torch.float64), steps, 0.9)
    assert not met.any() and (param == 1.0).all() and (rec == 0.5).all() and (below == 0.5 * 15 / 16).all()


# ---- the interface -----------------------------------------------------------------------------------------------------------
def test_bindings_and_exports():
    import sageattention_amd as sa
    from sageattention_amd import _build, _lib as L, core
    _build.build()
    lib = L.lib()
    assert lib.sage_abi_version() == 3
    P = ctypes.POINTER(L.SageTensor)
    i, f, p, i64 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64
    assert L.SIGNATURES["sage_attn_tile_mass"] == (i, [P, P, p, p, i, i, i, i, i, i, i, i, i, f, i, p, p])
    assert L.SIGNATURES["sage_block_plan_recall"] == (i, [p, i64, p, i, i, i, i, p, p, p])
    assert lib.sage_attn_tile_mass.argtypes == L.SIGNATURES["sage_attn_tile_mass"][1]
    assert lib.sage_block_plan_recall.argtypes == L.SIGNATURES["sage_block_plan_recall"][1]
    for name in ("sageattn_tile_mass", "plan_recall", "sparge_tune"):
        assert name in sa.__all__ and name in core.__all__ and getattr(sa, name) is getattr(core, name)
    sig = inspect.signature(sa.sageattn_tile_mass)
    assert list(sig.parameters) == ["q", "k", "tensor_layout", "sm_scale", "qk_quant_gran", "smooth_k"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[2:]] == ["HND", None, "per_thread", True]
    assert list(inspect.signature(sa.plan_recall).parameters) == ["plan_or_map", "mass"]
    sig = inspect.signature(sa.sparge_tune)
    assert list(sig.parameters) == ["q", "k", "tensor_layout", "target", "rule", "simthreshd1", "keep_first", "keep_last", "steps",
                                    "reduce", "sm_scale", "qk_quant_gran", "mass"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[2:]] == ["HND", 0.95, "cdf", 0.6, 0, 0, 8, "mean", None,
                                                                             "per_thread", None]
    assert sa.SpargeTuning.__slots__ == ("rule", "param", "met", "recall", "recall_below", "density")


def test_python_arguments_are_checked_before_any_tensor_is_touched():
    import sageattention_amd as sa
    x = object()  # not a tensor: any access would raise something else
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="target"):
            sa.sparge_tune(x, x, target=bad)
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="steps"):
            sa.sparge_tune(x, x, steps=bad)
    with pytest.raises(ValueError, match="rule"):
        sa.sparge_tune(x, x, rule="top")
    with pytest.raises(ValueError, match="reduce"):
        sa.sparge_tune(x, x, reduce="max")
    with pytest.raises(ValueError, match="keep_first"):
        sa.sparge_tune(x, x, keep_first=-1)
    with pytest.raises(ValueError, match="qk_quant_gran"):
        sa.sparge_tune(x, x, qk_quant_gran="per_block")
    with pytest.raises(ValueError, match="layout"):
        sa.sparge_tune(x, x, tensor_layout="BHND")
    with pytest.raises(ValueError, match="qk_quant_gran"):
        sa.sageattn_tile_mass(x, x, qk_quant_gran="per_block")
    with pytest.raises(ValueError, match="layout"):
        sa.sageattn_tile_mass(x, x, tensor_layout="DNH")
    with pytest.raises(ValueError, match="mass"):
        sa.plan_recall(x, x)
    mass = torch.zeros(2, 2, 2, 10)
    with pytest.raises(ValueError, match="mass"):
        sa.plan_recall(x, mass.double())
    with pytest.raises(TypeError):
        sa.plan_recall(x, mass)
    with pytest.raises(ValueError, match="does not match"):
        sa.plan_recall(torch.ones(2, 2, 2, 9, dtype=torch.bool), mass)
    with pytest.raises(ValueError, match="plan was made for"):
        sa.plan_recall(sa.BlockSparsePlan(torch.zeros(8, dtype=torch.int32), 2, 2, 300, 616), mass)


# ---- the C entry points check their arguments before any launch (fake device addresses: only where no GPU is visible, where
#      every launch attempt returns SAGE_ERR_LAUNCH = -5, as tests/test_pvskip.py does it)
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")
FAKE, ODD4, ODD16 = 1 << 20, (1 << 20) + 2, (1 << 20) + 4


def _mass(**change):
    from sageattention_amd import _build, _lib as L
    _build.build()
    t = L.SageTensor(FAKE, 1 << 16, 1 << 12, 64)
    args = dict(q=t, k=t, qs=FAKE, ks=FAKE, B=1, Hq=2, Hk=1, M=200, N=616, D=64, gran=3, blkq=128, warpq=32, sm=0.125, lm1=0,
                mass=FAKE, stream=None)
    args.update(change)
    return L.lib().sage_attn_tile_mass(*[args[n] for n in "q k qs ks B Hq Hk M N D gran blkq warpq sm lm1 mass stream".split()])


def _recall(**change):
    from sageattention_amd import _build, _lib as L
    _build.build()
    args = dict(lists=FAKE, lbytes=1 << 20, mass=FAKE, B=1, Hq=2, M=200, N=616, recall=FAKE, kept=FAKE, stream=None)
    args.update(change)
    return L.lib().sage_block_plan_recall(*[args[n] for n in "lists lbytes mass B Hq M N recall kept stream".split()])


@no_gpu
def test_tile_mass_checks_before_the_launch():
    from sageattention_amd import _lib as L
    assert _mass() == -5                               # the control: a valid call reaches the launch
    assert _mass(gran=2) == -5 and _mass(D=128) == -5 and _mass(M=1, N=1) == -5 and _mass(lm1=1, sm=0.0) == -5
    assert _mass(gran=2, ks=ODD16) == -5               # per_warp reads its k scales one by one
    for name in ("q", "k", "qs", "ks", "mass"):        # SAGE_ERR_INVALID_ARGUMENT
        assert _mass(**{name: None}) == -1, name
    for name in ("qs", "ks", "mass"):
        assert _mass(**{name: ODD4}) == -1, name
    assert _mass(ks=ODD16) == -1                       # per_thread: four scales in one 16-byte load
    assert _mass(q=L.SageTensor(FAKE + 8, 1 << 16, 1 << 12, 64)) == -1
    assert _mass(k=L.SageTensor(FAKE, 1 << 16, 1 << 12, 72)) == -1
    assert _mass(M=0) == -1 and _mass(N=0) == -1 and _mass(Hq=3, Hk=2) == -1
    assert _mass(sm=0.0) == -1 and _mass(sm=float("nan")) == -1
    assert _mass(gran=0) == -1 and _mass(gran=4) == -1 and _mass(blkq=96) == -1 and _mass(warpq=48) == -1
    assert _mass(D=96) == -2                           # SAGE_ERR_UNSUPPORTED_HEAD_DIM
    assert _mass(gran=1) == -3                         # SAGE_ERR_UNSUPPORTED: per_block, as the sparse operators refuse it
    assert _mass(mass=None, D=96) == -1                # the argument statuses come first


@no_gpu
def test_plan_recall_checks_before_the_launch():
    from sageattention_amd import _lib as L
    need = L.lib().sage_block_sparse_workspace_bytes(1, 2, 200, 616)
    assert _recall() == -5 and _recall(lbytes=need) == -5
    for name in ("lists", "mass", "recall", "kept"):
        assert _recall(**{name: None}) == -1, name
    for name in ("mass", "recall", "kept"):
        assert _recall(**{name: ODD4}) == -1, name
    assert _recall(lists=ODD16) == -1                  # list rows are read 16 bytes aligned, as by the attention kernels
    assert _recall(lbytes=need - 4) == -1
    assert _recall(B=0) == -1 and _recall(M=0) == -1 and _recall(N=-1) == -1


# ---- the GPU test's tolerance sees two planted mistakes ------------------------------------------------------------------------
def _tile_mass_cases():
    import test_calib_gpu as G
    B, Hq, Hk, M, N = G.MAIN
    return [(kind, D, gran, dtype, M, N) for kind in ("firm", "normal") for D in (64, 128) for gran in ("per_warp", "per_thread")
            for dtype in (torch.float16, torch.bfloat16)]


@pytest.mark.parametrize("case", _tile_mass_cases(), ids=lambda c: "-".join(str(x).replace("torch.", "") for x in c))
def test_the_gpu_tolerance_sees_the_planted_mistakes(case):
    """on the inputs of the GPU test: keys >= N counted in the last tile, and 1/128 instead of 1/c_i, both move entries by
    more than the tolerance the kernel is held to -- by a wide margin, so the tolerance is no loophole for either"""
    import test_calib_gpu as G
    kind, D, gran, dtype, M, N = case
    logits, ref = G.reference(*case)
    tol = G.tolerance(ref, logits, N)
    assert 4e-4 <= G.eps_for(logits, N) <= 8e-4  # "about 5e-4" at these shapes
    for wrong in (C.tile_mass_counts_padding, C.tile_mass_weights_128):
        excess = ((wrong(logits, M, N) - ref).abs() / tol).max()
        assert float(excess) > 10.0, (wrong.__name__, float(excess))
    # the first mistake shows in the ragged tile of every q-block, the second in every tile of the ragged q-block
    assert (((C.tile_mass_counts_padding(logits, M, N) - ref).abs() > tol)[..., -1]).all()
    assert (((C.tile_mass_weights_128(logits, M, N) - ref).abs() > tol)[:, :, -1]).all()
