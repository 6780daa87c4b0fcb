"""Shared-prefix attention on the paged cache (``sageattn_splitkv_paged_prefix``, include/sageattn_hip_prefix.h) without a GPU:
the new header against its ctypes table, the workspace formula, the C status table of the two entry points, the Python
refusals, the torch.library ops and the restatement of the rule in tests/prefix_util.py.  What the kernels compute:
test_prefix_gpu.py."""
import ctypes
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import prefix_util as XU
import seqpar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = "sageattention_amd_prefix"
OPS = ("attn_splitkv_paged_prefix", "attn_splitkv_paged_prefix_lse")
ENTRIES = ("sage_prefix_workspace_bytes", "sage_attn_fusedq_pv_f16_splitkv_paged_prefix",
           "sage_attn_fusedq_pv_f8_splitkv_paged_prefix")


# ---- 1. the new header against its table -----------------------------------------------------------------------------------------
def _prototypes(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    ctype = lambda s: re.sub(r"\bconst\b|\s", "", s)  # noqa: E731
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(sage_\w+)\s*\(([^()]*)\)\s*;", text):
        out[name] = (ctype(ret), [ctype(re.sub(r"\w+$", "", p.strip())) for p in params.split(",")])
    return out


def test_prefix_header_matches_its_table():
    from sageattention_amd import _lib as L
    protos = _prototypes("sageattn_hip_prefix.h")
    assert sorted(protos) == sorted(L.PREFIX_SIGNATURES) == sorted(ENTRIES)
    want = {"int": ctypes.c_int, "sage_stream_t": ctypes.c_void_p, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float}
    count = dict(zip(ENTRIES, (6, 34, 35)))
    for name, (ret, params) in protos.items():
        res, args = L.PREFIX_SIGNATURES[name]
        assert res is want[ret] and len(params) == len(args) == count[name], name
        for c, ct in zip(params, args):
            if c == "sage_tensor*":
                assert ct is ctypes.POINTER(L.SageTensor), (name, c)
            elif c.endswith("*"):
                assert c[:-1] in ("void", "float", "int32_t") and ct is ctypes.c_void_p, (name, c)
            else:
                assert ct is want[c], (name, c)
    # the two forms are the paged ones with the prefix arguments between kv_lens and the splits, without `causal`
    for pv in ("f16", "f8"):
        paged = L.PAGED_SIGNATURES[f"sage_attn_fusedq_pv_{pv}_splitkv_paged"][1]
        mine = L.PREFIX_SIGNATURES[f"sage_attn_fusedq_pv_{pv}_splitkv_paged_prefix"][1]
        k = len(paged) - 7                                     # ... kv_lens | num_splits causal q_fold ws ws_bytes stream
        assert mine[:k + 1] == paged[:k + 1] and mine[-4:] == paged[-4:]
    # the other headers and their tables are what they were
    assert len(L.SIGNATURES) == 69 and len(L.PAGED_SIGNATURES) == 3 and len(L.PAGED_ROWS_SIGNATURES) == 1
    assert not set(L.PREFIX_SIGNATURES) & (set(L.SIGNATURES) | set(L.KVCACHE_SIGNATURES) | set(L.PAGED_SIGNATURES)
                                           | set(L.PAGED_ROWS_SIGNATURES))
    for header in ("sageattn_hip.h", "sageattn_hip_kvcache.h", "sageattn_hip_paged.h", "sageattn_hip_paged_rows.h"):
        assert "_prefix(" not in open(os.path.join(ROOT, "include", header)).read()
    assert L.lib().sage_abi_version() == 3


def test_symbols_exported_and_bound():
    from sageattention_amd import _lib as L
    for name in ENTRIES:
        fn = getattr(L.lib(), name)
        assert fn.restype is L.PREFIX_SIGNATURES[name][0] and fn.argtypes == L.PREFIX_SIGNATURES[name][1]


# ---- 2. the workspace ----------------------------------------------------------------------------------------------------------
def test_workspace_bytes_is_its_formula():
    from sageattention_amd import _lib as L
    lib = L.lib()
    f, g = lib.sage_prefix_workspace_bytes, lib.sage_splitkv_workspace_bytes
    for B, H, M, D in ((1, 1, 1, 64), (3, 4, 8, 64), (3, 4, 48, 128), (32, 8, 4, 128), (5, 3, 7, 64)):
        for Sp in (1, 2, 3, 16):
            for Ss in (1, 5, 16):
                assert f(B, H, M, D, Sp, Ss) == g(1, H, B * M, D, Sp) + g(B, H, M, D, Ss) + 2 * B * H * M * 4 > 0
    for Sp, Ss in ((0, 1), (1, 0), (17, 1), (1, 17), (-1, 2), (2, -1)):
        assert f(3, 4, 8, 64, Sp, Ss) == 0
    for dims in ((0, 4, 8, 64), (3, 0, 8, 64), (3, 4, 0, 64), (3, 4, 8, 0), (-1, 4, 8, 64)):
        assert f(*dims, 2, 2) == 0


# ---- 3. the C status table -------------------------------------------------------------------------------------------------------
# Fake device addresses: where a GPU is visible a missed check would launch kernels on them, so this runs only where none
# is; there every launch attempt returns SAGE_ERR_LAUNCH (-5), which makes a launch observable (tests/test_cabi_symbols.py).
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="passes fake device addresses: only where no GPU is visible")
FAKE = 1 << 20
_TAIL = ("B Hq Hk M D gran warpq sm_scale table tstride max_pages page_size P lens ptable pmax plen km_p {}psplits num_splits "
         "q_fold ws ws_bytes stream")
_ARGS = {"f16": "q q_dt k8 v v_dt o o_dt ks km lse " + _TAIL.format(""),
         "f8": "q q_dt k8 v o o_dt ks km v_scale lse " + _TAIL.format("v_scale_p ")}
B_, HQ_, M_, D_ = 2, 4, 8, 64


def _pool(stride_n=64, data=FAKE):
    from sageattention_amd import _lib as L
    return L.SageTensor(data, 1 << 16, 1 << 13, stride_n)


def _nhd_q(B=B_, Hq=HQ_, M=M_, D=D_, data=FAKE):
    """an NHD-contiguous q [B, M, Hq, D] as a [B,H,N,D] descriptor: its folded view has one row stride"""
    from sageattention_amd import _lib as L
    return L.SageTensor(data, M * Hq * D, D, Hq * D)


def _ws_bytes(**kw):
    from sageattention_amd import _lib as L
    a = dict(B=B_, Hq=HQ_, M=M_, D=D_, psplits=3, num_splits=2)
    a.update(kw)
    return L.lib().sage_prefix_workspace_bytes(a["B"], a["Hq"], a["M"], a["D"], a["psplits"], a["num_splits"])


def _call(pv, **change):
    from sageattention_amd import _lib as L
    args = dict(q=_nhd_q(), q_dt=0, k8=_pool(), v=_pool(128 if pv == "f8" else 64), v_dt=0, o=_nhd_q(), o_dt=0, ks=FAKE, km=FAKE,
                v_scale=FAKE, lse=None, B=B_, Hq=HQ_, Hk=2, M=M_, D=D_, gran=3, warpq=32, sm_scale=0.125, table=FAKE, tstride=5,
                max_pages=5, page_size=128, P=24, lens=FAKE, ptable=FAKE, pmax=3, plen=FAKE, km_p=FAKE, v_scale_p=FAKE,
                psplits=3, num_splits=2, q_fold=2, ws=FAKE, ws_bytes=1 << 30, stream=None)
    args.update(change)
    return getattr(L.lib(), f"sage_attn_fusedq_pv_{pv}_splitkv_paged_prefix")(*[args[n] for n in _ARGS[pv].split()])


@no_gpu
@pytest.mark.parametrize("pv", ["f16", "f8"])
def test_valid_calls_reach_a_launch(pv):
    from sageattention_amd import _lib as L
    assert _call(pv) == -5
    assert _call(pv, ws_bytes=_ws_bytes()) == -5                                 # exactly the bytes of the formula
    assert _call(pv, lse=FAKE, q_fold=1, psplits=1, num_splits=16, ptable=FAKE + 4, plen=FAKE + 4, pmax=1,
                 ws_bytes=_ws_bytes(psplits=1, num_splits=16)) == -5
    assert _call(pv, page_size=256, v=_pool(256 if pv == "f8" else 64), D=128, q=_nhd_q(D=128), o=_nhd_q(D=128)) == -5
    # HND q with M = 1: the row stride of the folded view is stride_b; one sequence: any q
    assert _call(pv, M=1, q_fold=1, q=L.SageTensor(FAKE, HQ_ * D_, D_, D_)) == -5
    assert _call(pv, B=1, q=L.SageTensor(FAKE, 1 << 16, M_ * D_, D_)) == -5


@no_gpu
@pytest.mark.parametrize("pv", ["f16", "f8"])
def test_status_table(pv):
    """Each argument made invalid on its own returns its argument status: nothing was launched (a launch returns -5 here)."""
    from sageattention_amd import _lib as L
    odd = L.SageTensor(FAKE + 8, M_ * HQ_ * D_, D_, HQ_ * D_)
    hnd = L.SageTensor(FAKE, HQ_ * M_ * D_, M_ * D_, D_)      # HND-contiguous with M = 8: no single row stride
    cases = [
        # what is the prefix's own
        (dict(ptable=None), -1), (dict(ptable=FAKE + 2), -1), (dict(ptable=FAKE + 1), -1), (dict(plen=None), -1),
        (dict(plen=FAKE + 2), -1), (dict(plen=FAKE + 3), -1), (dict(pmax=0), -1), (dict(pmax=-2), -1), (dict(km_p=None), -3),
        (dict(km_p=FAKE + 8), -3), (dict(psplits=0), -1), (dict(psplits=17), -1), (dict(q=hnd), -3),
        (dict(pmax=1 << 24, page_size=256, v=_pool(256 if pv == "f8" else 64)), -4),
        (dict(B=1 << 16, M=1 << 15, q_fold=1), -4),
        # q_fold, always read: the suffix pass is causal
        (dict(q_fold=0), -1), (dict(q_fold=3), -1), (dict(q_fold=-1), -1),
        # the workspace: one byte short of the formula, misaligned, missing
        (dict(ws_bytes=_ws_bytes() - 1), -1), (dict(ws_bytes=16), -1), (dict(ws_bytes=0), -1), (dict(ws=None), -1),
        (dict(ws=FAKE + 8), -1),
        # head_dim and page size
        (dict(D=96), -2), (dict(D=32), -2), (dict(page_size=32), -1), (dict(page_size=96), -1), (dict(page_size=512), -1),
        # what the paged entries answer for the arguments they share
        (dict(table=None), -1), (dict(table=FAKE + 2), -1), (dict(max_pages=0), -1), (dict(P=0), -1), (dict(tstride=4), -1),
        (dict(lens=None), -1), (dict(lens=FAKE + 2), -1), (dict(q=None), -1), (dict(k8=None), -1), (dict(v=None), -1),
        (dict(o=None), -1), (dict(ks=None), -1), (dict(km=None), -3), (dict(q=odd), -1), (dict(km=FAKE + 8), -3),
        (dict(q_dt=2), -1), (dict(o_dt=2), -1), (dict(num_splits=0), -1), (dict(num_splits=17), -1), (dict(gran=1), -3),
        (dict(gran=0), -1), (dict(warpq=24), -1), (dict(sm_scale=0.0), -1), (dict(B=0), -1), (dict(Hq=0), -1), (dict(Hk=0), -1),
        (dict(M=0), -1), (dict(Hq=3), -1)]
    cases += ([(dict(v_scale=None), -1), (dict(v_scale_p=None), -1), (dict(v_scale_p=FAKE + 8), -1)] if pv == "f8"
              else [(dict(v_dt=2), -1)])
    wrong = [(sorted(c), st, got) for c, st in cases if (got := _call(pv, **c)) != st]
    assert not wrong, wrong


# ---- 4. Python refusals, raised before any device call ---------------------------------------------------------------------------
def _cpu_whole(pv="fp16", D=64, layout="HND", page_size=128, P=8, nseq=3, rows=False):
    """a cache of ``nseq`` sequences with zero state on the CPU"""
    import sageattention_amd as sa
    shape = (P, 2, page_size, D) if layout == "HND" else (P, page_size, 2, D)
    z = lambda s, dt: torch.zeros(s, dtype=dt)  # noqa: E731
    if rows:
        c = sa.SagePagedRowCache(pv, "per_thread", layout, 2.0, page_size, torch.float16)
        c.k_tail = z((nseq, 2, 2, 64, D), torch.float16)
        if pv != "fp8":
            c.v_pool = z(shape, torch.float16)
    else:
        c = sa.SagePagedKVCache(z(shape, torch.float16), z(shape, torch.float16), pv, "per_thread", layout, 2.0)
    c.k8, c.k_scale, c.km = z(shape, torch.int8), z((P, 2, page_size // 64 * 4), torch.float32), z((nseq, 2, D), torch.float16)
    if pv == "fp8":
        c.v8 = z((P, 2, D, page_size) if layout == "HND" else (P, D, 2, page_size), torch.uint8).view(torch.float8_e4m3fn)
        c.v_scale, c.v_coef = z((nseq, 2, D), torch.float32), z((nseq, 2, 2, D), torch.float32)
    return c


def test_refusals():
    import sageattention_amd as sa
    from sageattention_amd import prefix as X
    assert "sageattn_splitkv_paged_prefix" in sa.__all__ and sa.sageattn_splitkv_paged_prefix is X.sageattn_splitkv_paged_prefix
    f = sa.sageattn_splitkv_paged_prefix
    whole = _cpu_whole()
    pre, suf = whole.narrow(0, 1), whole.narrow(1, 2)
    q = torch.zeros(2, 4, 8, 64, dtype=torch.float16)
    table, lens = torch.zeros(2, 3, dtype=torch.int32), torch.tensor([80, 3], dtype=torch.int32)
    ptable, plen = torch.zeros(2, dtype=torch.int32), torch.tensor([200], dtype=torch.int32)
    # caches that do not share pools, named
    other = _cpu_whole()
    with pytest.raises(ValueError, match="share pools.*k8"):
        f(q, suf, table, lens, other.narrow(0, 1), ptable, plen)
    moved = whole.narrow(0, 1)
    moved.k_scale = whole.k_scale.clone()
    with pytest.raises(ValueError, match="share pools.*k_scale"):
        f(q, suf, table, lens, moved, ptable, plen)
    moved = whole.narrow(0, 1)
    moved.v = whole.v[:4]
    with pytest.raises(ValueError, match="share pools.* v pools"):
        f(q, suf, table, lens, moved, ptable, plen)
    moved = whole.narrow(0, 1)
    moved.k8 = whole.k8.transpose(1, 2).contiguous().transpose(1, 2)             # the shape, other strides
    with pytest.raises(ValueError, match="share pools.*k8"):
        f(q, suf, table, lens, moved, ptable, plen)
    w8 = _cpu_whole(pv="fp8")
    moved = w8.narrow(0, 1)
    moved.v8 = w8.v8.clone()
    with pytest.raises(ValueError, match="share pools.*v8"):
        f(q, w8.narrow(1, 2), table, lens, moved, ptable, plen)
    # mismatched pv / granularity / layout / dtype
    with pytest.raises(ValueError, match="share pools: pv"):
        f(q, suf, table, lens, w8.narrow(0, 1), ptable, plen)
    for name, value in (("qk_quant_gran", "per_warp"), ("tensor_layout", "NHD")):
        moved = whole.narrow(0, 1)
        setattr(moved, name, value)
        with pytest.raises(ValueError, match=f"share pools: {name}"):
            f(q, suf, table, lens, moved, ptable, plen)
    rows16 = _cpu_whole(rows=True)           # (a cache that owns its pools keeps its dtype as an attribute)
    rows_bf = rows16.narrow(0, 1)
    rows_bf.dtype = torch.bfloat16
    with pytest.raises(ValueError, match="share pools: dtype"):
        f(q, rows16.narrow(1, 2), table, lens, rows_bf, ptable, plen)
    # a prefix with two sequences; a suffix cache of another batch size
    with pytest.raises(ValueError, match="one sequence"):
        f(q, suf, table, lens, whole.narrow(0, 2), ptable, plen)
    with pytest.raises(ValueError, match="sequences"):
        f(q, whole, torch.zeros(2, 3, dtype=torch.int32), lens, pre, ptable, plen)
    for bad in (torch.zeros(2, 2, 3), object(), None):
        with pytest.raises(TypeError, match="SagePagedKVCache or a SagePagedRowCache"):
            f(q, suf, table, lens, bad, ptable, plen)
    # the prefix's table and length
    with pytest.raises(TypeError, match="prefix_table"):
        f(q, suf, table, lens, pre, [0, 1], plen)
    with pytest.raises(TypeError, match="prefix_table must be of dtype int32"):
        f(q, suf, table, lens, pre, ptable.long(), plen)
    for bad in (torch.zeros(2, 2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(1, 1, 2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="prefix_table shape"):
            f(q, suf, table, lens, pre, bad, plen)
    with pytest.raises(ValueError, match="prefix_table must be contiguous"):
        f(q, suf, table, lens, pre, torch.zeros(4, dtype=torch.int32)[::2], plen)
    with pytest.raises(ValueError, match="prefix_table is on"):
        f(q, suf, table, lens, pre, ptable.to("meta"), plen)
    with pytest.raises(TypeError, match="prefix_len"):
        f(q, suf, table, lens, pre, ptable, 200)
    with pytest.raises(TypeError, match="prefix_len must be of dtype int32"):
        f(q, suf, table, lens, pre, ptable, plen.long())
    for bad in (torch.zeros(2, dtype=torch.int32), torch.zeros((), dtype=torch.int32)):
        with pytest.raises(ValueError, match="prefix_len shape"):
            f(q, suf, table, lens, pre, ptable, bad)
    # what sageattn_splitkv_paged refuses
    with pytest.raises(TypeError, match="kv_lens"):
        f(q, suf, table, None, pre, ptable, plen)
    with pytest.raises(ValueError, match="kv_lens shape"):
        f(q, suf, table, torch.zeros(3, dtype=torch.int32), pre, ptable, plen)
    with pytest.raises(ValueError, match="block_table shape"):
        f(q, suf, torch.zeros(3, 3, dtype=torch.int32), lens, pre, ptable, plen)
    for name in ("num_splits", "prefix_splits"):
        for bad in (0, 17, -1):
            with pytest.raises(ValueError, match=name):
                f(q, suf, table, lens, pre, ptable, plen, **{name: bad})
        with pytest.raises(TypeError, match=name):
            f(q, suf, table, lens, pre, ptable, plen, **{name: 2.0})
    with pytest.raises(TypeError, match="q_fold"):
        f(q, suf, table, lens, pre, ptable, plen, q_fold=2.0)
    for bad in (0, 3, -1):
        with pytest.raises(ValueError, match="q_fold"):
            f(q, suf, table, lens, pre, ptable, plen, q_fold=bad)
    with pytest.raises(ValueError, match="head_dim"):
        f(torch.zeros(2, 4, 8, 128, dtype=torch.float16), suf, table, lens, pre, ptable, plen)
    with pytest.raises(ValueError, match="dtype"):
        f(q.bfloat16(), suf, table, lens, pre, ptable, plen)
    with pytest.raises(ValueError, match="divisible"):
        f(torch.zeros(2, 3, 8, 64, dtype=torch.float16), suf, table, lens, pre, ptable, plen)


# ---- 5. the torch.library ops ------------------------------------------------------------------------------------------------------
def test_ops_live_in_their_own_namespace():
    import sageattention_amd  # noqa: F401
    import sageattention_amd.ops  # noqa: F401
    names = torch._C._dispatch_get_all_op_names()
    assert sorted(n.split("::")[1] for n in names if n.startswith(NS + "::")) == sorted(OPS)
    assert len([n for n in names if n.startswith("sageattention_amd::")]) == 26
    assert len([n for n in names if n.startswith("sageattention_amd_paged::")]) == 5
    assert len([n for n in names if n.startswith("sageattention_amd_paged_rows::")]) == 1
    params = ("Tensor q, Tensor k8, Tensor k_scale, Tensor km, Tensor v, Tensor? v_scale, Tensor block_table, Tensor kv_lens, "
              "Tensor prefix_table, Tensor prefix_len, Tensor km_p, Tensor? v_scale_p, SymInt num_splits, SymInt prefix_splits, "
              "SymInt q_fold, str tensor_layout, float sm_scale, str qk_quant_gran")
    for name in OPS:
        s = str(getattr(getattr(torch.ops, NS), name).default._schema)
        assert params in s and "!" not in s, s
        assert s.endswith("-> (Tensor, Tensor)" if name.endswith("_lse") else "-> Tensor")


@pytest.mark.parametrize("rows", [False, True], ids=["bound", "rows"])
@pytest.mark.parametrize("layout", ["HND", "NHD"])
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_fakes_describe_their_outputs(layout, pv, rows):
    """o contiguous in q's shape and dtype -- for a strided q as well --, lse fp32 [B, Hq, M] contiguous"""
    import sageattention_amd as sa
    with FakeTensorMode():
        D, B, HQ, M = 128, 2, 4, 8
        whole = _cpu_whole(pv=pv, D=D, layout=layout, nseq=B + 1, rows=rows)
        for name, t in list(vars(whole).items()):
            if isinstance(t, torch.Tensor):
                setattr(whole, name, torch.empty(t.shape, dtype=t.dtype, device="cuda"))
        pre, suf = whole.narrow(0, 1), whole.narrow(1, B)
        lens = torch.empty((B,), dtype=torch.int32, device="cuda")
        table = torch.empty((B, 3), dtype=torch.int32, device="cuda")
        ptable = torch.empty((1, 2), dtype=torch.int32, device="cuda")
        plen = torch.empty((1,), dtype=torch.int32, device="cuda")
        qshape = (B, HQ, M, D) if layout == "HND" else (B, M, HQ, D)
        big = torch.empty(tuple(2 * s for s in qshape), dtype=torch.float16, device="cuda")
        contiguous = torch.empty(qshape).stride()
        for q in (torch.empty(qshape, dtype=torch.float16, device="cuda"), big[:B, ::2, :qshape[2], D:]):
            o = sa.sageattn_splitkv_paged_prefix(q, suf, table, lens, pre, ptable, plen, q_fold=4)
            assert isinstance(o, torch.Tensor) and o.shape == q.shape and o.dtype == q.dtype and o.stride() == contiguous
            o, lse = sa.sageattn_splitkv_paged_prefix(q, suf, table, lens, pre, ptable[0], plen, 3, 2, return_lse=True)
            assert o.shape == q.shape and o.dtype == q.dtype and o.stride() == contiguous and o.device == q.device
            assert lse.shape == (B, HQ, M) and lse.dtype == torch.float32 and lse.is_contiguous() and lse.device == q.device


# ---- 6. the restatement of the rule --------------------------------------------------------------------------------------------------
def test_folded_rows_and_views():
    B, H, M, D = 3, 4, 5, 8
    q = torch.arange(B * H * M * D, dtype=torch.float32).reshape(B, H, M, D)
    qp = XU.fold_q(q, "HND")
    assert qp.shape == (1, H, B * M, D)
    flat_p, flat = qp.reshape(-1, D), q.reshape(-1, D)
    seen = set()
    for b in range(B):
        for h in range(H):
            for m in range(M):
                r = XU.folded_row(b, h, m, B, H, M)
                assert r == h * (B * M) + b * M + m and torch.equal(flat_p[r], flat[XU.native_row(b, h, m, B, H, M)])
                assert torch.equal(qp[0, h, b * M + m], q[b, h, m])
                seen.add(r)
    assert seen == set(range(B * H * M))
    assert torch.equal(XU.unfold_o(qp, B, "HND"), q)
    qn = q.transpose(1, 2).contiguous()
    qpn = XU.fold_q(qn, "NHD")
    assert qpn.shape == (1, B * M, H, D) and torch.equal(qpn.transpose(1, 2), qp) and qpn.data_ptr() == qn.data_ptr()
    assert torch.equal(XU.unfold_o(qpn, B, "NHD"), qn)
    lse = torch.arange(B * H * M, dtype=torch.float32).reshape(B, H, M)
    lse_p = lse.permute(1, 0, 2).reshape(1, H, B * M)
    assert torch.equal(XU.unfold_lse(lse_p, B), lse)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_combine_rule_against_the_bound(dtype):
    """the combine in torch fp32 on the merge case table (ordinary rows, equal rows, a dominant segment, a common offset of
    +-3e4, an empty segment filled with NaN / Inf, both empty): inside check_prefix's bound, and where one segment is empty
    the row keeps the other segment's bits"""
    rows, D = 8 * len(R.KINDS), 64
    cases = R.merge_cases(2, rows, D=D, dtype=dtype, seed=3)
    x = [o.float() + (torch.rand(o.shape, generator=torch.Generator().manual_seed(i)) - 0.5) * 0.25 * R.ulp(o.double(), dtype).float()
         for i, o in enumerate(cases.os)]                    # fp32 values that round to the case table's o: the kernel's o_x
    for xi, oi in zip(x, cases.os):
        fin = torch.isfinite(oi.float())
        xi[~fin] = oi.float()[~fin]
        assert torch.equal(xi.to(dtype)[fin], oi[fin])
    o, lse = XU.combine_rule(x[0], cases.lses[0], x[1], cases.lses[1], dtype)
    XU.check_prefix(o.view(1, 1, rows, D), lse.view(1, 1, rows), [c.view(1, 1, rows, D) for c in cases.os],
                    [l.view(1, 1, rows) for l in cases.lses], dtype)
    for name in ("e_first", "e_last"):
        m = cases.kind == R.KINDS.index(name)
        keep = 1 - R.kind_slot(name, 2)
        assert torch.equal(R.bits(o[m]), R.bits(cases.os[keep][m])) and torch.equal(lse[m], cases.lses[keep][m])
    m = cases.kind == R.KINDS.index("f")
    assert bool((o[m] == 0).all()) and bool(torch.isneginf(lse[m]).all())
