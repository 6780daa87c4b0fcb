"""The dense attention entry points without a GPU: which bad argument gives which status, with nothing launched.  All of them
go through attn_check (csrc/sage_attn.hip); the block-sparse, P.V-skip and predictor forms have their own tables
(test_block_sparse.py, test_pvskip.py, test_sparge.py).

The expected statuses in EXPECTED were recorded from the library built from the commit BEFORE attn_check took its arguments
as one block (the table below was run against that library and its answers written down), not from the code under test.
Where a case lists one status it held for every entry point that has the changed arguments; a dict gives the exceptions.

Not expressible through the C ABI, so not here: attn_mask together with is_causal or with FP8 P.V (the masked entry point
has neither argument)."""
import ctypes

import pytest
import torch

# Fake device addresses: where a GPU is visible a missed check would launch kernels on them, so this runs only where none
# is; there every launch attempt returns SAGE_ERR_LAUNCH (-5), which makes a launch observable (tests/test_cabi_symbols.py).
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")

FAKE = 1 << 20
ODD = FAKE + 8
BIG = 1 << 25  # keys: 2^19 tiles of 4 KiB reach the 2 GiB window of the 32-bit buffer offsets

_QK = "B Hq Hk M N D causal gran blkq warpq sm lm1 stream"
_FQ = "B Hq Hk M N D causal gran warpq sm stream"
_KT = "B Hq Hk M N D causal gran blkq warpq sm stream"
# variant -> (symbol, parameter names in order, fuse_q of the options or None)
_ENTRY = {
    "f16": ("sage_attn_qk_int8_pv_f16", "q k v vdt o odt qs ks vm lse " + _QK, None),
    "f8": ("sage_attn_qk_int8_pv_f8", "q k v o odt qs ks vs vm lse " + _QK, None),
    "varlen": ("sage_attn_qk_int8_pv_f16_varlen", "q k v vdt o odt qs ks cuq cuk " + _QK, None),
    "fusedq_f16": ("sage_attn_fusedq_pv_f16", "q qdt k v vdt o odt ks km vm lse " + _FQ, None),
    "fusedq_f8": ("sage_attn_fusedq_pv_f8", "q qdt k v o odt ks km vs vm lse " + _FQ, None),
    "masked": ("sage_attn_qk_int8_pv_f16_masked",
               "q k v vdt o odt qs ks mask mkind mstr lse B Hq Hk M N D gran blkq warpq sm lm1 stream", None),
    "f16_kvtiles": ("sage_attn_qk_int8_pv_f16_kvtiles", "q k v vdt o odt qs ks kvl lse " + _KT, None),
    "f8_kvtiles": ("sage_attn_qk_int8_pv_f8_kvtiles", "q k v o odt qs ks vs kvl lse " + _KT, None),
    "op_f16": ("sage_sageattn_pv_f16", "q k v dt o lse B Hq Hk M N D causal sm opts ws wsbytes stream", 0),
    "op_f16_fused": ("sage_sageattn_pv_f16", "q k v dt o lse B Hq Hk M N D causal sm opts ws wsbytes stream", 1),
    "op_f8": ("sage_sageattn_pv_f8", "q k v dt o lse B Hq Hk M N D causal sm smax opts ws wsbytes stream", 0),
    "op_f8_fused": ("sage_sageattn_pv_f8", "q k v dt o lse B Hq Hk M N D causal sm smax opts ws wsbytes stream", 1),
    # for the double faults only (its single faults: test_block_sparse.py)
    "f16_blocksparse": ("sage_attn_qk_int8_pv_f16_blocksparse", "q k v vdt o odt qs ks vm lse " + _QK[:-7] + " lists nbytes stream",
                        None),
}
_DENSE = [e for e in _ENTRY if e != "f16_blocksparse"]


def _tensor(data=FAKE, stride_n=64):
    from sageattention_amd import _lib as L
    return L.SageTensor(data, 1 << 16, 1 << 12, stride_n)


def _opts(fuse_q, gran=3, warpq=32, smooth_k=1, nwaves=0):
    from sageattention_amd import _lib as L
    return L.OpOpts(gran, warpq, smooth_k, fuse_q, nwaves)


def _kvl(k_tile=0, v_tile=0, ks_b=0, ks_h=0, ks_tile=0):
    from sageattention_amd import _lib as L
    return L.KvLayout(k_tile, v_tile, ks_b, ks_h, ks_tile)


def _valid(entry):
    fuse_q = _ENTRY[entry][2]
    t = _tensor()
    return dict(q=t, k=t, v=t, o=t, vdt=0, odt=0, qdt=0, dt=0, qs=FAKE, ks=FAKE, vs=FAKE, vm=None, km=FAKE, lse=None, B=1, Hq=2,
                Hk=1, M=200, N=333, D=64, causal=0, gran=3, blkq=128, warpq=32, sm=0.125, lm1=0, cuq=FAKE, cuk=FAKE, mask=FAKE,
                mkind=1, mstr=(ctypes.c_int64 * 4)(0, 0, 333, 1), kvl=_kvl(), smax=448.0,
                opts=None if fuse_q is None else _opts(fuse_q), ws=FAKE, wsbytes=1 << 40, lists=FAKE, nbytes=1 << 40, stream=None)


def _call(entry, **change):
    from sageattention_amd import _lib as L
    symbol, params, _ = _ENTRY[entry]
    args = dict(_valid(entry), **change)
    return getattr(L.lib(), symbol)(*[args[n] for n in params.split()])


def _single_faults():
    """(label, changed arguments): each applies to every dense entry point that has all of them"""
    nan, inf = float("nan"), float("inf")
    cases = []
    for n in "qkvo":  # a tensor without descriptor, without data, with an 8-byte-misaligned base
        cases += [(f"{n}=no descriptor", {n: None}), (f"{n}=null data", {n: _tensor(0)}), (f"{n}=misaligned", {n: _tensor(ODD)})]
    cases += [(f"{n}=null", {n: None}) for n in ("qs", "ks", "vs")]
    cases += [(f"{n}=misaligned", {n: ODD}) for n in ("vs", "vm", "km")]
    cases += [(f"{n}=0", {n: 0}) for n in ("B", "Hq", "Hk", "M", "N", "D")]
    cases += [("Hq % Hk != 0", dict(Hk=3)), ("D=96", dict(D=96))]
    cases += [(f"{n}={x}", {n: x}) for n in ("odt", "vdt", "qdt", "dt") for x in (-1, 2)]
    cases += [(f"gran={x}", dict(gran=x)) for x in (0, 1, 4)]  # 1 = per block: refused by the fused-Q forms only
    cases += [("blkq=96", dict(blkq=96)), ("warpq=24", dict(warpq=24)), ("warpq=64", dict(warpq=64)),
              ("blkq=64 warpq=64", dict(blkq=64, warpq=64)), ("blkq=64 warpq=128", dict(blkq=64, warpq=128))]
    cases += [(f"sm={x}", dict(sm=x)) for x in (0.0, -1.0, nan, inf)]
    cases += [(f"sm={x} lm1=1", dict(sm=x, lm1=1)) for x in (0.0, -1.0, nan)]
    cases += [("cuq=null", dict(cuq=None)), ("cuk=null", dict(cuk=None))]
    cases += [("mask=null", dict(mask=None)), ("mkind=0", dict(mkind=0)), ("mkind=4", dict(mkind=4)), ("mstr=null", dict(mstr=None))]
    cases += [("kvl=null", dict(kvl=None)), ("kvl k_tile<0", dict(kvl=_kvl(k_tile=-4096))), ("kvl v_tile<0", dict(kvl=_kvl(v_tile=-4096))),
              ("kvl ks_b<0", dict(kvl=_kvl(ks_b=-4, ks_h=24, ks_tile=4))), ("kvl ks_h<0", dict(kvl=_kvl(ks_b=48, ks_h=-4, ks_tile=4))),
              ("kvl ks_tile<0", dict(kvl=_kvl(ks_b=48, ks_h=24, ks_tile=-4))),
              ("kvl ks_tile<4 per_thread", dict(kvl=_kvl(ks_b=48, ks_h=24, ks_tile=2))),
              ("kvl k_tile misaligned", dict(kvl=_kvl(k_tile=4104))), ("kvl v_tile misaligned", dict(kvl=_kvl(v_tile=4100))),
              ("kvl ks_b misaligned per_thread", dict(kvl=_kvl(ks_b=50, ks_h=24, ks_tile=4))),
              ("kvl ks_h misaligned per_thread", dict(kvl=_kvl(ks_b=48, ks_h=26, ks_tile=4))),
              ("kvl ks_tile misaligned per_thread", dict(kvl=_kvl(ks_b=48, ks_h=24, ks_tile=6)))]
    # the three 2 GiB windows: K (rows of 64 bytes), V alone (K rows of 16 bytes keep K inside; V^T rows of N), the K scales alone
    cases += [("N=2^25: K window", dict(N=BIG)), ("N=2^25: V window", dict(N=BIG, k=_tensor(FAKE, 16), v=_tensor(FAKE, BIG))),
              ("N=2^25: k_scale window", dict(N=BIG, kvl=_kvl(k_tile=16, v_tile=16, ks_b=1 << 40, ks_h=1 << 32, ks_tile=4096)))]
    # the one-call operators' own arguments
    cases += [("opts=null", dict(opts=None)), ("ws=null", dict(ws=None)), ("ws=misaligned", dict(ws=ODD)), ("wsbytes=64", dict(wsbytes=64)),
              ("smax=0", dict(smax=0.0)), ("smax<0", dict(smax=-1.0)), ("smax=nan", dict(smax=nan))]
    return cases


def _op_option_faults():
    """(label, entry, changed arguments): bad fields of sage_op_opts, per fuse_q"""
    out = []
    for entry in ("op_f16", "op_f16_fused", "op_f8", "op_f8_fused"):
        f = _ENTRY[entry][2]
        out += [("opts smooth_k=0", entry, dict(opts=_opts(f, smooth_k=0))), ("opts gran=1", entry, dict(opts=_opts(f, gran=1))),
                ("opts gran=4", entry, dict(opts=_opts(f, gran=4))), ("opts warpq=24", entry, dict(opts=_opts(f, warpq=24))),
                ("opts warpq=64", entry, dict(opts=_opts(f, warpq=64))), ("opts nwaves=3", entry, dict(opts=_opts(f, nwaves=3)))]
    return out


def _double_faults():
    """(label, entry, changed arguments): two faults with different statuses, or two checks of one status in a fixed order"""
    return [("D=96 + q=no descriptor", "f16", dict(D=96, q=None)), ("D=96 + odt=2", "f16", dict(D=96, odt=2)),
            ("D=96 + sm=0", "f8", dict(D=96, sm=0.0)), ("D=96 + N=2^25", "f16", dict(D=96, N=BIG)),
            ("Hq % Hk != 0 + N=2^25", "f8", dict(Hk=3, N=BIG)), ("gran=1 + q=misaligned", "fusedq_f16", dict(gran=1, q=_tensor(ODD))),
            ("qdt=2 + gran=1", "fusedq_f8", dict(qdt=2, gran=1)), ("cuq=null + D=96", "varlen", dict(cuq=None, D=96)),
            ("kvl k_tile<0 + N=2^25", "f16_kvtiles", dict(kvl=_kvl(k_tile=-4096), N=BIG)),
            ("mkind=0 + D=96", "masked", dict(mkind=0, D=96)), ("causal + lists=null", "f16_blocksparse", dict(causal=1, lists=None)),
            ("causal + D=96", "f16_blocksparse", dict(causal=1, D=96)), ("dt=2 + ws=null", "op_f16_fused", dict(dt=2, ws=None)),
            ("D=96 + opts smooth_k=0", "op_f8", dict(D=96, opts=_opts(0, smooth_k=0)))]


def all_cases():
    """-> [(label, entry, changed arguments)]"""
    out = []
    for label, change in _single_faults():
        out += [(label, e, change) for e in _DENSE if set(change) <= set(_ENTRY[e][1].split())]
    return out + _op_option_faults() + _double_faults()


# label -> status, or {entry: status, None: status of the others}
EXPECTED = {
    'q=no descriptor': -1,
    'q=null data': -1,
    'q=misaligned': -1,
    'k=no descriptor': -1,
    'k=null data': -1,
    'k=misaligned': -1,
    'v=no descriptor': -1,
    'v=null data': -1,
    'v=misaligned': -1,
    'o=no descriptor': -1,
    'o=null data': -1,
    'o=misaligned': -1,
    'qs=null': -1,
    'ks=null': -1,
    'vs=null': -1,
    'vs=misaligned': -1,
    'vm=misaligned': -1,
    'km=misaligned': -3,
    'B=0': -1,
    'Hq=0': -1,
    'Hk=0': -1,
    'M=0': -1,
    'N=0': -1,
    'D=0': -2,
    'Hq % Hk != 0': -1,
    'D=96': -2,
    'odt=-1': -1,
    'odt=2': -1,
    'vdt=-1': -1,
    'vdt=2': -1,
    'qdt=-1': -1,
    'qdt=2': -1,
    'dt=-1': -1,
    'dt=2': -1,
    'gran=0': -1,
    'gran=1': {None: -5, 'fusedq_f16': -3, 'fusedq_f8': -3},
    'gran=4': -1,
    'blkq=96': -1,
    'warpq=24': -1,
    'warpq=64': -5,
    'blkq=64 warpq=64': -5,
    'blkq=64 warpq=128': -1,
    'sm=0.0': -1,
    'sm=-1.0': -1,
    'sm=nan': -1,
    'sm=inf': -1,
    'sm=0.0 lm1=1': -5,
    'sm=-1.0 lm1=1': -5,
    'sm=nan lm1=1': -5,
    'cuq=null': -1,
    'cuk=null': -1,
    'mask=null': -1,
    'mkind=0': -1,
    'mkind=4': -1,
    'mstr=null': -1,
    'kvl=null': -1,
    'kvl k_tile<0': -1,
    'kvl v_tile<0': -1,
    'kvl ks_b<0': -1,
    'kvl ks_h<0': -1,
    'kvl ks_tile<0': -1,
    'kvl ks_tile<4 per_thread': -1,
    'kvl k_tile misaligned': -1,
    'kvl v_tile misaligned': -1,
    'kvl ks_b misaligned per_thread': -1,
    'kvl ks_h misaligned per_thread': -1,
    'kvl ks_tile misaligned per_thread': -1,
    'N=2^25: K window': -4,
    'N=2^25: V window': -4,
    'N=2^25: k_scale window': -4,
    'opts=null': -1,
    'ws=null': -1,
    'ws=misaligned': -1,
    'wsbytes=64': -1,
    'smax=0': -1,
    'smax<0': -1,
    'smax=nan': -1,
    'opts smooth_k=0': -3,
    'opts gran=1': -1,
    'opts gran=4': -1,
    'opts warpq=24': -1,
    'opts warpq=64': -1,
    'opts nwaves=3': -1,
    'D=96 + q=no descriptor': -1,
    'D=96 + odt=2': -2,
    'D=96 + sm=0': -1,
    'D=96 + N=2^25': -2,
    'Hq % Hk != 0 + N=2^25': -1,
    'gran=1 + q=misaligned': -3,
    'qdt=2 + gran=1': -1,
    'cuq=null + D=96': -1,
    'kvl k_tile<0 + N=2^25': -1,
    'mkind=0 + D=96': -1,
    'causal + lists=null': -1,
    'causal + D=96': -3,
    'dt=2 + ws=null': -1,
    'D=96 + opts smooth_k=0': -2,
}


def expected(label, entry):
    want = EXPECTED[label]
    return want.get(entry, want.get(None)) if isinstance(want, dict) else want


@no_gpu
def test_valid_calls_reach_a_launch():
    assert [e for e in _ENTRY if _call(e) != -5] == []


@no_gpu
def test_every_dense_entry_point_has_the_shared_cases():
    """The table is not empty where it matters: every dense entry point sees the faults of the tensors, the shape, head_dim,
    sm_scale and the K window."""
    seen = {}
    for label, entry, _ in all_cases():
        seen.setdefault(entry, set()).add(label)
    shared = {"q=misaligned", "k=null data", "v=no descriptor", "o=misaligned", "B=0", "Hq % Hk != 0", "D=96", "sm=nan",
              "N=2^25: K window"}
    assert [e for e in _DENSE if not shared <= seen[e]] == []
    assert len(all_cases()) > 500


@no_gpu
def test_status_table():
    """Each bad argument returns the status the library returned before the refactor, and none of them is a launch (-5)
    unless it was one then (an accepted value, such as per-block scales on the forms that take them)."""
    wrong = [(label, entry, expected(label, entry), got) for label, entry, change in all_cases()
             if (got := _call(entry, **change)) != expected(label, entry)]
    assert not wrong, wrong


def test_recorded_launches_are_valid_values():
    """The table's only launches (-5) are values the entry point accepts: per-block scales on the forms that take them, a
    Q scale group of 64 rows, and any sm_scale when the caller says that the logit multiplier is one.  Every fault is refused."""
    valid = {"gran=1", "warpq=64", "blkq=64 warpq=64", "sm=0.0 lm1=1", "sm=-1.0 lm1=1", "sm=nan lm1=1"}
    launched = {label for label, entry, _ in all_cases() if expected(label, entry) == -5}
    assert launched == valid
