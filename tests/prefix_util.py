"""The rule of shared-prefix attention (include/sageattn_hip_prefix.h) restated for the tests: where a query row lives in the
folded prefix pass, the combine of the two segments in torch, and the bound of the general case against the fp64 merge of the
two existing operators' results.  CPU only; nothing of the library."""
import torch

import seqpar_ref as R
from splitkv_util import merged_reference


# ---- folded rows -----------------------------------------------------------------------------------------------------------
def folded_row(b, h, m, B, H, M):
    """row of (b, h, m) in the slots of the prefix pass, [H, B * M]"""
    return (h * B + b) * M + m


def native_row(b, h, m, B, H, M):
    """... and in the slots of the suffix pass and in lse, [B, H, M]"""
    return (b * H + h) * M + m


def fold_q(q, layout):
    """the q of the prefix pass, [1, H, B * M, D] (NHD: [1, B * M, H, D]): q_p[0, h, b * M + m] = q[b, h, m]"""
    if layout == "NHD":
        B, M, H, D = q.shape
        return q.reshape(1, B * M, H, D)
    B, H, M, D = q.shape
    return q.permute(1, 0, 2, 3).reshape(1, H, B * M, D)


def unfold_o(o_p, B, layout):
    """o of the prefix pass back in q's shape"""
    if layout == "NHD":
        _, BM, H, D = o_p.shape
        return o_p.reshape(B, BM // B, H, D)
    _, H, BM, D = o_p.shape
    return o_p.reshape(H, B, BM // B, D).permute(1, 0, 2, 3).contiguous()


def unfold_lse(lse_p, B):
    """lse [1, H, B * M] of the prefix pass as [B, H, M]"""
    _, H, BM = lse_p.shape
    return lse_p.reshape(H, B, BM // B).permute(1, 0, 2).contiguous()


# ---- the combine, in torch fp32 ----------------------------------------------------------------------------------------------
def combine_rule(o_p, L_p, o_s, L_s, dtype):
    """Step 3 of the rule on fp32 segment results o_x [rows, D], L_x [rows] (natural log, the segment's own correction in it,
    -inf = no key): one fp32 torch operation per operation of the rule, in its order.  -> (o in ``dtype``, lse fp32)"""
    o_p, o_s, L_p, L_s = o_p.float(), o_s.float(), L_p.float(), L_s.float()
    ninf = float("-inf")
    mx = torch.maximum(L_p, L_s)
    use_p, use_s = L_p != ninf, L_s != ninf
    zero = torch.zeros_like(mx)
    w_p = torch.where(use_p, torch.exp(torch.where(use_p, L_p - mx, zero)), zero)
    w_s = torch.where(use_s, torch.exp(torch.where(use_s, L_s - mx, zero)), zero)
    total = w_p + w_s                      # (a dropped weight is 0 here, and 0 + w is exact)
    acc = torch.where(use_p.unsqueeze(-1), torch.nan_to_num(o_p) * w_p.unsqueeze(-1), torch.zeros_like(o_p))
    acc = torch.where(use_s.unsqueeze(-1), acc + torch.nan_to_num(o_s) * w_s.unsqueeze(-1), acc)
    some = total > 0
    inv = torch.where(some, 1.0 / torch.where(some, total, torch.ones_like(total)), zero)
    o = (acc * inv.unsqueeze(-1)).to(dtype)
    lse = torch.where(some, mx + torch.log(torch.where(some, total, torch.ones_like(total))), torch.full_like(mx, ninf))
    return o, lse


# ---- the general case --------------------------------------------------------------------------------------------------------
# fp32 operations of the combine on the path of one output element that merge_tolerances (seqpar_ref.py) does not name:
# o_x * w_x, the two additions of the accumulator (the first, to 0, is exact; counting it covers the second-order terms of
# (1 + u)^k - 1, as sum_additions does), w_p + w_s, 1 / (w_p + w_s) and the final product
O_ROUNDINGS = 6
# ... and on the path of lse: w_p + w_s, and logf's own rounding of a value of at most ln 2 in magnitude
LSE_ROUNDINGS = 2


def check_prefix(o, lse, seg_o, seg_lse, dtype):
    """o [B,H,M,D], lse [B,H,M] (or None) of the shared-prefix operator against the fp64 merge of ``seg_o`` = (o_p, o_s) and
    ``seg_lse`` = (lse_p, lse_s): what the two EXISTING operators return for the segments, the prefix one on the folded q and
    un-folded, each o in ``dtype``, each lse the natural log with the segment's correction in it, -inf without a key.

    The bound, term by term.  The kernel merges each segment's splits with the arithmetic of the existing merge, so its L_x
    are the operators' lse_x bit for bit and its fp32 o_x round to the operators' o_x: |o_x - y_x| <= ulp(y_x) / 2.  The second
    level is then a two-slot merge on natural-log LSEs of fp32 inputs, which is what merged_reference and check_merge bound:
      * check_merge: eps * sum_x w_x |o_x| + ulp(ref) / 2, eps = EPS_EXP + 3 * 2^-24 * (1 + max |L_x|) -- the exp / log pair,
        the rounding of L_x - mx (relative error |L_x - mx| * 2^-24 <= 2 max |L_x| * 2^-24 in w_x) and of mx + log(.);
      * merged_reference: sum_x w_x ulp(y_x) / 2 for the unrounded o_x, and the binade edge of the final rounding;
      * here: O_ROUNDINGS * 2^-24 * sum_x w_x |o_x| for the fp32 operations of the combine counted above, every intermediate
        being at most sum_x w_x |o_x| in magnitude after normalisation; LSE_ROUNDINGS * 2^-24 on lse.
    No term comes from a run of the kernel."""
    D = o.shape[-1]
    og = o.detach().cpu().reshape(-1, D)
    ref, o_extra = merged_reference(list(seg_o), list(seg_lse), dtype, og)
    R.check_merge(og, None, ref, dtype, o_extra=o_extra + O_ROUNDINGS * R.U32 * ref.wabs)
    if lse is not None:
        lg = lse.detach().cpu().reshape(-1)
        _, l_tol = R.merge_tolerances(ref, None)
        l_tol = l_tol + LSE_ROUNDINGS * R.U32
        assert not torch.isnan(lg).any()
        assert torch.equal(torch.isneginf(lg), torch.isneginf(ref.lse))
        fin = torch.isfinite(ref.lse)
        e = (lg.double() - ref.lse).abs()
        assert (e[fin] <= l_tol[fin]).all(), (e[fin] / l_tol[fin]).max().item()
    return ref
