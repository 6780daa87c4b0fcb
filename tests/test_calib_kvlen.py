"""Calibration with per-batch key lengths, without a GPU: the three twins are exported with the declared signatures, the two
new C entry points are bound as the header declares them and refuse what they must before any launch, ``kv_lens`` and the
keywords are checked before any tensor is touched, and the three functions without lengths keep refusing the keyword."""
import ctypes
import inspect

import pytest
import torch


# ---- the interface -----------------------------------------------------------------------------------------------------------
def test_bindings_and_exports():
    import sageattention_amd as sa
    from sageattention_amd import _build, _lib as L, core
    _build.build()
    lib = L.lib()
    assert lib.sage_abi_version() == 3
    P = ctypes.POINTER(L.SageTensor)
    i, f, p, i64 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64
    # the arguments of the twin, then kv_lens in front of the stream
    for name in ("sage_attn_tile_mass", "sage_block_plan_recall"):
        res, args = L.SIGNATURES[name]
        assert L.SIGNATURES[name + "_kvlen"] == (res, args[:-1] + [p, args[-1]])
        assert getattr(lib, name + "_kvlen").argtypes == L.SIGNATURES[name + "_kvlen"][1]
    assert L.SIGNATURES["sage_attn_tile_mass_kvlen"] == (i, [P, P, p, p, i, i, i, i, i, i, i, i, i, f, i, p, p, p])
    assert L.SIGNATURES["sage_block_plan_recall_kvlen"] == (i, [p, i64, p, i, i, i, i, p, p, p, p])
    for name in ("sageattn_tile_mass_kvlen", "plan_recall_kvlen", "sparge_tune_kvlen"):
        assert name in sa.__all__ and name in core.__all__ and getattr(sa, name) is getattr(core, name)
    sig = inspect.signature(sa.sageattn_tile_mass_kvlen)
    assert list(sig.parameters) == ["q", "k", "kv_lens", "tensor_layout", "sm_scale", "qk_quant_gran"]  # no smooth_k
    assert [sig.parameters[n].default for n in list(sig.parameters)[3:]] == ["HND", None, "per_thread"]
    assert list(inspect.signature(sa.plan_recall_kvlen).parameters) == ["plan_or_map", "mass", "kv_lens"]
    sig = inspect.signature(sa.sparge_tune_kvlen)
    assert list(sig.parameters) == ["q", "k", "kv_lens", "tensor_layout", "target", "rule", "simthreshd1", "keep_first",
                                    "keep_last", "steps", "reduce", "sm_scale", "qk_quant_gran", "mass"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[3:]] == ["HND", 0.95, "cdf", 0.6, 0, 0, 8, "mean", None,
                                                                             "per_thread", None]
    # the twin of sparge_tune has its keywords and defaults
    ref = inspect.signature(sa.sparge_tune).parameters
    assert {n: sig.parameters[n].default for n in ref if n not in ("q", "k")} == {n: ref[n].default for n in ref
                                                                                  if n not in ("q", "k")}


def test_the_docstrings_state_the_reductions_and_point_at_each_other():
    import sageattention_amd as sa
    for fn, twin in ((sa.sageattn_tile_mass, "sageattn_tile_mass_kvlen"), (sa.plan_recall, "plan_recall_kvlen"),
                     (sa.sparge_tune, "sparge_tune_kvlen")):
        assert twin in fn.__doc__ and "kv_lens" in fn.__doc__
    doc = sa.sparge_tune_kvlen.__doc__
    for phrase in ("valid[:, None, None]", "nv.clamp(min=1)", ".amin((0, 2))", "kept.sum((0, 2))", "k_smooth_quant_kvlen",
                   "the K pre-pass still runs"):
        assert phrase in doc, phrase


def test_kv_lens_is_checked_before_any_tensor_is_touched():
    import sageattention_amd as sa
    x = object()  # not a tensor: any access would raise something else
    mass = torch.zeros(2, 2, 2, 10)
    calls = (lambda lens: sa.sageattn_tile_mass_kvlen(x, x, lens), lambda lens: sa.plan_recall_kvlen(x, x, lens),
             lambda lens: sa.sparge_tune_kvlen(x, x, lens))
    for call in calls:
        for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(2), [3, 4], None):
            with pytest.raises(TypeError, match="kv_lens"):
                call(bad)
        for bad in (torch.zeros(2, 1, dtype=torch.int32), torch.zeros((), dtype=torch.int32)):
            with pytest.raises(ValueError, match="kv_lens"):
                call(bad)
    # [B] needs the batch count: the first thing read of q (a CPU tensor here: nothing is launched) or of the mass
    q = torch.zeros(2, 2, 128, 64, dtype=torch.float16)
    three = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"kv_lens shape \(3,\) does not match \[B=2\]"):
        sa.sageattn_tile_mass_kvlen(q, q, three)
    with pytest.raises(ValueError, match=r"kv_lens shape \(3,\) does not match \[B=2\]"):
        sa.sparge_tune_kvlen(q, q, three)
    with pytest.raises(ValueError, match=r"kv_lens shape \(3,\) does not match \[B=2\]"):
        sa.plan_recall_kvlen(torch.ones(2, 2, 2, 10, dtype=torch.bool), mass, three)


def test_python_arguments_are_checked_before_any_tensor_is_touched():
    """the argument checks of sparge_tune, sageattn_tile_mass and plan_recall, repeated for the twins"""
    import sageattention_amd as sa
    x = object()
    lens = torch.zeros(2, dtype=torch.int32)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="target"):
            sa.sparge_tune_kvlen(x, x, lens, target=bad)
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="steps"):
            sa.sparge_tune_kvlen(x, x, lens, steps=bad)
    with pytest.raises(ValueError, match="rule"):
        sa.sparge_tune_kvlen(x, x, lens, rule="top")
    with pytest.raises(ValueError, match="reduce"):
        sa.sparge_tune_kvlen(x, x, lens, reduce="max")
    with pytest.raises(ValueError, match="keep_first"):
        sa.sparge_tune_kvlen(x, x, lens, keep_first=-1)
    with pytest.raises(ValueError, match="keep_last"):
        sa.sparge_tune_kvlen(x, x, lens, keep_last=1.5)
    with pytest.raises(ValueError, match="qk_quant_gran"):
        sa.sparge_tune_kvlen(x, x, lens, qk_quant_gran="per_block")
    with pytest.raises(ValueError, match="layout"):
        sa.sparge_tune_kvlen(x, x, lens, tensor_layout="BHND")
    with pytest.raises(ValueError, match="qk_quant_gran"):
        sa.sageattn_tile_mass_kvlen(x, x, lens, qk_quant_gran="per_block")
    with pytest.raises(ValueError, match="layout"):
        sa.sageattn_tile_mass_kvlen(x, x, lens, tensor_layout="DNH")
    with pytest.raises(TypeError, match="smooth_k"):
        sa.sageattn_tile_mass_kvlen(x, x, lens, smooth_k=False)
    with pytest.raises(ValueError, match="mass"):
        sa.plan_recall_kvlen(x, x, lens)
    mass = torch.zeros(2, 2, 2, 10)
    with pytest.raises(ValueError, match="mass"):
        sa.plan_recall_kvlen(x, mass.double(), lens)
    with pytest.raises(TypeError):
        sa.plan_recall_kvlen(x, mass, lens)
    with pytest.raises(ValueError, match="does not match"):
        sa.plan_recall_kvlen(torch.ones(2, 2, 2, 9, dtype=torch.bool), mass, lens)
    with pytest.raises(ValueError, match="plan was made for"):
        sa.plan_recall_kvlen(sa.BlockSparsePlan(torch.zeros(8, dtype=torch.int32), 2, 2, 300, 616), mass, lens)


def test_the_functions_without_lengths_still_refuse_the_keyword():
    from sageattention_amd import core
    q = torch.zeros(1, 1, 128, 64, dtype=torch.float16)
    lens = torch.tensor([64], dtype=torch.int32)
    with pytest.raises(TypeError, match="kv_lens"):
        core.sageattn_tile_mass(q, q, kv_lens=lens)
    with pytest.raises(TypeError, match="kv_lens"):
        core.plan_recall(torch.ones(1, 1, 1, 2, dtype=torch.bool), torch.zeros(1, 1, 1, 2), kv_lens=lens)
    with pytest.raises(TypeError, match="kv_lens"):
        core.sparge_tune(q, q, kv_lens=lens)
    for fn in (core.sageattn_tile_mass, core.plan_recall, core.sparge_tune):
        assert "kv_lens" not in inspect.signature(fn).parameters


# ---- the C entry points check their arguments before any launch (fake device addresses: only where no GPU is visible, where
#      every launch attempt returns SAGE_ERR_LAUNCH = -5, as tests/test_calib.py does it).  Both forms are called: the twin
#      without lengths is the yardstick for every status but that of kv_lens itself.
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")
FAKE, ODD4, ODD16 = 1 << 20, (1 << 20) + 2, (1 << 20) + 4
MASS_ARGS = "q k qs ks B Hq Hk M N D gran blkq warpq sm lm1 mass".split()
RECALL_ARGS = "lists lbytes mass B Hq M N recall kept".split()


def _mass(kvlen, **change):
    from sageattention_amd import _build, _lib as L
    _build.build()
    t = L.SageTensor(FAKE, 1 << 16, 1 << 12, 64)
    args = dict(q=t, k=t, qs=FAKE, ks=FAKE, B=3, Hq=2, Hk=1, M=200, N=616, D=64, gran=3, blkq=128, warpq=32, sm=0.125, lm1=0,
                mass=FAKE, lens=FAKE, stream=None)
    args.update(change)
    if kvlen:
        return L.lib().sage_attn_tile_mass_kvlen(*[args[n] for n in MASS_ARGS + ["lens", "stream"]])
    return L.lib().sage_attn_tile_mass(*[args[n] for n in MASS_ARGS + ["stream"]])


def _recall(kvlen, **change):
    from sageattention_amd import _build, _lib as L
    _build.build()
    args = dict(lists=FAKE, lbytes=1 << 20, mass=FAKE, B=3, Hq=2, M=200, N=616, recall=FAKE, kept=FAKE, lens=FAKE, stream=None)
    args.update(change)
    if kvlen:
        return L.lib().sage_block_plan_recall_kvlen(*[args[n] for n in RECALL_ARGS + ["lens", "stream"]])
    return L.lib().sage_block_plan_recall(*[args[n] for n in RECALL_ARGS + ["stream"]])


@no_gpu
def test_tile_mass_kvlen_checks_before_the_launch():
    from sageattention_amd import _lib as L
    valid = [dict(), dict(gran=2), dict(D=128), dict(M=1, N=1), dict(lm1=1, sm=0.0), dict(gran=2, ks=ODD16), dict(lens=ODD16)]
    for change in valid:
        assert _mass(True, **change) == -5 and _mass(False, **change) == -5, change   # reaches the launch
    assert _mass(True, lens=None) == -1 and _mass(True, lens=ODD4) == -1              # SAGE_ERR_INVALID_ARGUMENT
    assert _mass(True, lens=None, D=96) == -1 and _mass(True, lens=None, gran=1) == -1
    faults = [{name: None} for name in ("q", "k", "qs", "ks", "mass")] + [{name: ODD4} for name in ("qs", "ks", "mass")]
    faults += [dict(ks=ODD16), dict(q=L.SageTensor(FAKE + 8, 1 << 16, 1 << 12, 64)), dict(k=L.SageTensor(FAKE, 1 << 16, 1 << 12, 72)),
               dict(M=0), dict(N=0), dict(B=0), dict(Hq=3, Hk=2), dict(sm=0.0), dict(sm=float("nan")), dict(gran=0), dict(gran=4),
               dict(blkq=96), dict(warpq=48), dict(D=96), dict(gran=1), dict(mass=None, D=96)]
    for change in faults:
        want = _mass(False, **change)
        assert want in (-1, -2, -3), change
        assert _mass(True, **change) == want, change
    assert _mass(True, D=96) == -2 and _mass(True, gran=1) == -3


@no_gpu
def test_plan_recall_kvlen_checks_before_the_launch():
    from sageattention_amd import _lib as L
    need = L.lib().sage_block_sparse_workspace_bytes(3, 2, 200, 616)
    for change in (dict(), dict(lbytes=need), dict(lens=ODD16)):
        assert _recall(True, **change) == -5 and _recall(False, **change) == -5, change
    assert _recall(True, lens=None) == -1 and _recall(True, lens=ODD4) == -1
    faults = [{name: None} for name in ("lists", "mass", "recall", "kept")] + [{name: ODD4} for name in ("mass", "recall", "kept")]
    faults += [dict(lists=ODD16), dict(lbytes=need - 4), dict(B=0), dict(Hq=0), dict(M=0), dict(N=-1)]
    for change in faults:
        assert _recall(False, **change) == -1, change
        assert _recall(True, **change) == -1, change
