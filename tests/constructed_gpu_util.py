"""Device-side helpers shared by the constructed-operand GPU tests (tests/test_constructed_logits_gpu.py,
tests/test_constructed_subsets_gpu.py, tests/test_constructed_masks_gpu.py): a case's operands in the form the C entry points take."""
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
