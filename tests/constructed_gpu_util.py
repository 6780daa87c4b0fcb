"""Device-side helpers shared by the constructed-operand GPU tests (tests/test_constructed_logits_gpu.py,
tests/test_constructed_subsets_gpu.py, tests/test_constructed_masks_gpu.py, tests/test_constructed_layouts_gpu.py): a case's, or a
stack's, operands in the form the C entry points take."""
import torch

import constructed_cases as C

GRAN_CODE = {"per_block": 1, "per_warp": 2, "per_thread": 3}


class _Dev:
    """one case's operands on the device, in the form the entry points take"""

    def __init__(self, sa, c, pv):
        self.c, self.pv = c, pv
        self.q8, self.k8 = c["q8"].cuda(), c["k8"].cuda()
        self.qs, self.ks = c["q_scale"].cuda(), c["k_scale"].cuda()
        self.qs_folded = (c["q_scale"] * c["logit_mult"]).cuda()  # exact: a power of two
        self.v_scale = None
        if pv == "fp8":
            perm = sa.quant.fp8_token_order()
            nblk = c["v_f8t"].shape[-1] // 64
            idx = (torch.arange(nblk).view(-1, 1) * 64 + perm.view(1, -1)).reshape(-1)  # position -> token
            self.v = c["v_f8t"].view(torch.uint8)[..., idx].contiguous().view(torch.float8_e4m3fn).cuda()
            self.v_scale = c["v_scale"].cuda()
        else:
            self.v = C.v_of(c, pv).cuda()
        self.code = GRAN_CODE[c["gran"]]

    def out(self):
        c = self.c
        return torch.full((C.B, C.HQ, c["M"], c["D"]), float("nan"), dtype=C.OUT_DTYPE[self.pv], device="cuda")

    def dense(self, sa):
        c, o = self.c, self.out()
        if self.pv == "fp8":
            lse = sa._qattn._attn_f8(self.q8, self.k8, self.v, o, self.qs, self.ks, self.v_scale, None, 1, c["causal"],
                                     self.code, c["sm_scale"], 1)
        elif c["gran"] == "per_block":
            lse = sa._qattn._attn_f16(self.q8, self.k8, self.v, o, self.qs_folded, self.ks, None, 1, c["causal"], self.code,
                                      c["sm_scale"], 1, logit_mult_is_one=True)
        else:
            lse = sa._qattn._attn_f16(self.q8, self.k8, self.v, o, self.qs, self.ks, None, 1, c["causal"], self.code,
                                      c["sm_scale"], 1)
        torch.cuda.synchronize()
        return o, lse


def _desc(L, t):
    return L.SageTensor(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))


def _pinned(nw):
    """context: the geometry pinned to nw waves, restored on exit"""
    from sageattention_amd import _lib as L

    class _Pin:
        def __enter__(self):
            assert L.lib().sage_set_tuning(0, nw) == 0

        def __exit__(self, *exc):
            L.lib().sage_set_tuning(0, 0)
    return _Pin()


def fp8_kernel_order(sa, v8):
    """uint8 e4m3 V^T [..., 64 k] with the tokens in natural order -> the order the kernels read (quant.fp8_token_order inside
    every block of 64)"""
    perm = sa.quant.fp8_token_order()
    idx = (torch.arange(v8.shape[-1] // 64).view(-1, 1) * 64 + perm.view(1, -1)).reshape(-1)  # position -> token
    return v8[..., idx].contiguous()


class _StackDev:
    """a stacked call's operands (constructed_cases.stack) on the device, for the int8-Q entry points through the C ABI.
    ``lens``: per-batch key lengths; K rows beyond them hold int8 127, the K scales of the tiles wholly beyond them NaN, fp16 /
    bf16 V rows NaN, the e4m3 V^T zeros up to the end of the last tile and 0x7F behind it (tests/test_constructed_subsets_gpu.py)"""

    def __init__(self, sa, st, pv, lens=None):
        from sageattention_amd import _lib as L
        self.L, self.st, self.pv = L, st, pv
        self.B, self.Hq, self.Hk, N = st["Bs"], st["Hq"], st["Hk"], st["N"]
        self.lens = [N] * self.B if lens is None else [min(int(n), N) for n in lens]
        self.q8, self.qs = st["q8"].cuda(), st["q_scale"].cuda()
        self.qs_folded = (st["q_scale"] * st["logit_mult"]).cuda()  # exact: a power of two
        k8, ks = st["k8"].clone(), st["k_scale"].clone()
        per = ks.shape[-1] // ((N + 63) // 64)
        for b, n in enumerate(self.lens):
            k8[b, :, n:] = 127
            ks[b, :, (n + 63) // 64 * per:] = float("nan")
        self.k8, self.ks = k8.cuda(), ks.cuda()
        self.v_scale = None
        if pv == "fp8":
            v8 = st["v_f8t"].view(torch.uint8).clone()
            for b, n in enumerate(self.lens):
                v8[b, :, :, n:] = 0
                v8[b, :, :, (n + 63) // 64 * 64:] = 0x7F
            self.v = fp8_kernel_order(sa, v8).view(torch.float8_e4m3fn).cuda()
            self.v_scale = st["v_scale"].cuda()
        else:
            v = C.v_of(st, pv).clone()
            for b, n in enumerate(self.lens):
                v[b, :, n:] = float("nan")
            self.v = v.cuda()
        self.kv_lens = torch.tensor(self.lens, dtype=torch.int32, device="cuda")
        self.code = GRAN_CODE[st["gran"]]

    def out(self):
        st = self.st
        o = torch.full((self.B, self.Hq, st["M"], st["D"]), float("nan"), dtype=C.OUT_DTYPE[self.pv], device="cuda")
        return o, torch.full((self.B, self.Hq, st["M"]), float("nan"), device="cuda")

    def run(self, name="", causal=False, lists=None, kv_lens=False, nw=None, cpu=True):
        """sage_attn_qk_int8_pv_{f16,f8}[_<name>] -> (o, lse2), both NaN beforehand.  per_block with FP16 / BF16 V goes in with
        logit_mult_is_one and the folded q scales, as _Dev.dense does"""
        L, st = self.L, self.st
        o, lse = self.out()
        fold = st["gran"] == "per_block" and self.pv != "fp8"
        head = (_desc(L, self.q8), _desc(L, self.k8), _desc(L, self.v))
        mid = (_desc(L, o), L.dtype_code(o.dtype), (self.qs_folded if fold else self.qs).data_ptr(), self.ks.data_ptr())
        warpq = 128 if st["gran"] == "per_block" else 32
        tail = (None, lse.data_ptr(), self.B, self.Hq, self.Hk, st["M"], st["N"], st["D"], int(causal), self.code, 128, warpq,
                st["sm_scale"], int(fold))
        if lists is not None:
            tail += (lists.data_ptr(), lists.numel() * 4)
            if kv_lens:
                tail += (None, None)  # pv_thresh, skipped: the kernel without the P.V skip
        if kv_lens:
            tail += (self.kv_lens.data_ptr(),)
        tail += (L.stream_ptr(o.device),)
        sym = "sage_attn_qk_int8_pv_" + ("f8" if self.pv == "fp8" else "f16") + ("_" + name if name else "")
        call = lambda: (getattr(L.lib(), sym)(*head, *mid, self.v_scale.data_ptr(), *tail) if self.pv == "fp8" else
                        getattr(L.lib(), sym)(*head, L.dtype_code(self.v.dtype), *mid, *tail))
        if nw is None:
            L.check(call(), sym)
        else:
            with _pinned(nw):
                L.check(call(), sym)
        torch.cuda.synchronize()
        return (o.cpu(), lse.cpu()) if cpu else (o, lse)
