"""CPU proof that the bound of tests/constructed_cases.py is sound and has teeth.  Nothing here looks at a kernel.

Soundness: on every case the GPU test runs, the oracle's restatement of the kernel ("hip" flavour of attn_tile_loop: the
same roundings of P, the same row sums, fp32 accumulation) stays within ``bound`` of the fp64 reference.
Teeth: a float64 restatement of the loop that makes ONE deliberate mistake leaves the bound on the family meant to catch
that mistake.  Closed forms: the reference itself is checked against values known without computing a softmax."""
import math

import numpy as np
import pytest
import torch

import constructed_cases as C

_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    if _RECORD:
        print("\noracle (hip flavour) on the constructed cases: largest |err| / bound   [o, lse2]")
        for (fam, pv, D), (ro, rl) in sorted(_RECORD.items()):
            print(f"  {fam:13s} {pv:5s} D={D:<4d} {ro:6.3f} {rl:6.3f}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("family", C.FAMILIES)
def test_oracle_within_bound(family, pv, D):
    """ratio <= 1 for every element of every case; the scales of ramp / extreme_s / one_hot are uniform, so the
    granularity changes nothing the oracle sees there and one is enough."""
    grans = C.GRANS if family in ("scale_ladder", "coarse_lsb", "big_v") else ("per_warp",)
    worst = (0.0, 0.0)
    for label, c in C.family_cases(family, D, pv, grans):
        o, lse2 = C.oracle(c, pv)
        ro, rl = C.ratios(c, pv, o, lse2)
        assert ro <= 1.0 and rl <= 1.0, (label, ro, rl)
        worst = (max(worst[0], ro), max(worst[1], rl))
    _RECORD[(family, pv, D)] = worst


def _mutant_ratio(c, pv, mistake):
    o, lse2 = C.restate64(c, pv, mistake)
    return max(C.ratios(c, pv, o, lse2))


# (mistake, family that must catch it, builder).  head_dim 64 unless the mistake needs 128.
TEETH = [
    ("swap_key_groups", "scale_ladder", lambda: C.scale_ladder(64, 456, False, "per_thread")),
    ("tile3_scales_of_tile2", "scale_ladder", lambda: C.scale_ladder(64, 456, False, "per_thread")),
    ("tile3_scales_of_tile2", "scale_ladder", lambda: C.scale_ladder(64, 456, False, "per_warp")),
    ("tile3_scales_of_tile2", "scale_ladder", lambda: C.scale_ladder(128, 320, True, "per_block")),
    ("q_group_xor_1", "scale_ladder", lambda: C.scale_ladder(64, 456, False, "per_thread")),
    ("q_group_xor_1", "scale_ladder", lambda: C.scale_ladder(128, 456, False, "per_warp")),
    ("q_group_xor_1", "scale_ladder", lambda: C.scale_ladder(64, 456, False, "per_block")),
    ("drop_last_key", "one_hot", lambda: C.one_hot(64, 456, False, "per_warp", "last")),
    ("drop_last_key", "one_hot", lambda: C.one_hot(128, 456, False, "per_warp", "last", subnormal=True)),
    ("admit_key_N", "extreme_s", lambda: C.extreme_s(64, 456, False, "per_warp", "zero")),
    ("wrap_2_21", "extreme_s", lambda: C.extreme_s(128, 456, False, "per_warp", "corner")),
    ("clamp_p_2_5", "ramp", lambda: C.ramp(64, 456, False, "per_warp", "6", "ascending")),
    ("clamp_p_2_5", "ramp", lambda: C.ramp(128, 320, False, "per_warp", "6", "sawtooth")),
]


@pytest.mark.parametrize("i", range(len(TEETH)), ids=[f"{m}-{f}-{k}" for k, (m, f, _) in enumerate(TEETH)])
def test_bound_has_teeth(i):
    """each deliberate mistake exceeds the bound (ratio > 1) for every PV type it applies to"""
    mistake, family, build = TEETH[i]
    c = build()
    # P never exceeds 2^3 (times the offset) under FP8 PV: a clamp at 2^5 is no mistake there
    pvs = ("fp16", "bf16") if mistake == "clamp_p_2_5" else C.PVS
    for pv in pvs:
        clean = max(C.ratios(c, pv, *C.restate64(c, pv)))
        r = _mutant_ratio(c, pv, mistake)
        print(f"teeth: {mistake:22s} on {family:12s} {c['gran']:10s} D={c['D']:<3d} {pv:5s} ratio {r:12.1f}   (no mistake: {clean:.1e})")
        assert clean < 1e-3, (pv, clean)   # the restatement without the mistake IS the reference
        assert r > 1.0, (mistake, family, pv, r)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_zero_q_reference_is_the_mean(D, causal):
    c = C.extreme_s(D, 456, causal, "per_warp", "zero")
    for pv in C.PVS:
        ref = C.reference64(c, pv)
        V = C.v64(c, pv)
        if causal:
            n = torch.arange(1, 457, dtype=torch.float64)
            want, want_l = V.cumsum(2) / n.view(1, 1, -1, 1), torch.log2(n).view(1, 1, -1).expand(1, 2, -1)
        else:
            want, want_l = V.mean(2, keepdim=True).expand(1, 2, 150, D), torch.full((1, 2, 150), math.log2(456), dtype=torch.float64)
        assert (ref["o"] - want).abs().max() < 1e-13 and (ref["lse2"] - want_l).abs().max() < 1e-13


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("where", C.ONE_HOT_KEYS)
def test_one_hot_reference_is_the_v_row(D, where):
    """o = V[hot] to within 1 output ulp and lse2 = the hot logit (the 455 others together weigh 455 * 2^-78)"""
    for causal in (False, True):
        c = C.one_hot(D, 456, causal, "per_thread", where)
        hot = c["hot"]
        rows = slice(hot, None) if causal else slice(None)
        logit = (D * c["r"].double() * 127 * 2.0 ** -12).view(1, 1, -1)
        for pv in C.PVS:
            ref, V = C.reference64(c, pv), C.v64(c, pv)
            want = V[:, :, hot:hot + 1]
            assert ((ref["o"] - want).abs() <= C.out_ulp(want, pv))[:, :, rows].all()
            assert (ref["lse2"] - logit)[:, :, rows].abs().max() < 1e-12


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("shape", C.RAMP_SHAPES)
def test_ramp_is_rank_one_and_hits_its_steps_exactly(D, shape):
    for step, units in C.RAMP_UNITS.items():
        c = C.ramp(D, 512, False, "per_thread", step, shape)
        S = (c["q8"].to(torch.int64) @ c["k8"].to(torch.int64).transpose(2, 3))  # exact integers
        assert torch.equal(S[0, 0], c["r"].to(torch.int64).view(-1, 1) * c["K"].view(1, -1))
        assert S.abs().max() < 2 ** 22
        # fp32, associated as the kernel does: (q_scale * logit_mult) * k_scale, times float(S)
        sc = (c["q_scale_rows"] * torch.tensor(c["logit_mult"])).unsqueeze(-1) * c["k_scale_cols"].unsqueeze(2)
        t = S.float() * sc
        assert t.dtype == torch.float32 and torch.equal(t.double(), S.double() * 2.0 ** -12)
        steep = t[0, 0, 0].view(8, 64).amax(-1)              # row 0 has r = 4: the steepest trend
        assert c["r"][0] == 4
        levels = torch.tensor(C._ramp_levels(shape, 8), dtype=torch.float32)
        want = torch.tensor(np.float32(units) / np.float32(1024))  # 0.5, thr - 2^-10, thr, thr + 2^-10, 40: exact in fp32
        assert float(want) * 1024 == units
        d_t, d_l = steep[1:] - steep[:-1], levels[1:] - levels[:-1]  # fp32 subtraction, exact
        assert torch.equal(d_t, d_l * want)
        # every 32-row wave holds every trend, both signs
        for w0 in range(0, 150 - 31, 32):
            assert set(c["r"][w0:w0 + 32].tolist()) == {4, -4, 2, -2, 1, -1, 0}


def test_extreme_scores_are_the_corners():
    c = C.extreme_s(128, 456, False, "per_warp", "corner")
    S = C.scores(c)
    assert S.max() == 2 ** 21 and S.min() == -2080768
    assert torch.equal(S[0, 0, 0, :64].unique(), torch.tensor([-2080768.0, 2097152.0], dtype=torch.float64))
    assert abs(float((S.max() - S.min()) * C.scale_matrix(c).max()) - 15.94) < 0.01
    c = C.extreme_s(64, 456, False, "per_warp", "corner")
    assert C.scores(c).max() == 2 ** 20 and C.scores(c).min() == -1040384


def test_coarse_lsb_and_delta():
    """the row LSB is what the family says, and delta is 0.75 s for small scores, 0.875 s at S = 2^21"""
    for e in (-6, -5, -4):
        assert float(C.row_lsb(C.coarse_lsb(64, 456, False, "per_thread", e)).max()) == 2.0 ** e
    assert float(C.row_lsb(C.scale_ladder(64, 456, False, "per_thread")).max()) == 2.0 ** -12
    assert (C.BIAS + 2 ** 21) * 2.0 ** -24 == 0.875 and C.BIAS * 2.0 ** -24 == 0.75


def test_logit_mult_is_a_power_of_two_in_fp32():
    assert np.float32(C.SM_SCALE) * np.float32(1.4426950408889634) == np.float32(0.125) == np.float32(C.LOGIT_MULT)
