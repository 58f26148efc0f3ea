"""The checker of the int8 stage tests (oracle/i8_select.py) catches what it claims to catch.

tests/i8_select_cases.py: FakeLaunch is a NumPy stand-in for the kernels around the int8 collect scan -- sample select, collect
predicate, select_i8 with its three stages and the certificate, the bf16 fallback -- that produces every buffer the checker reads
from small clustered operands.  The checker passes on it in each configuration (anchored thresholds, key budget 1, margin 0 with
k = 1, the bf16 sample form), and each single seeded fault fails on the property it belongs to.  No GPU."""
import numpy as np
import pytest

from oracle import i8_select as S
from tests.i8_select_cases import CONFIGS, FAULTS, FakeLaunch


@pytest.fixture(scope="module")
def launches():
    return {c: FakeLaunch(c) for c in CONFIGS}


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_checker_passes_on_a_correct_launch(launches, config):
    f = launches[config]
    rep = S.check_launch(f, f.opts, final=f.final, stats=f.stats)
    assert rep["worst_cos_err"] <= (1.5e-6 if config == "equality" else 1e-7) and rep["widest_bracket"] <= 1      # (equality plants a cosine 1e-6 off)
    assert rep["certified"] + rep["uncertified"] == rep["B"]


def test_the_stand_in_reaches_the_edges_the_faults_need(launches):
    """anchored thresholds and thresholds left at the m-th sample score, negative thresholds, a pool past its cap, lists past theirs,
    certified and uncertified queries, the worst case of the two-eps cut, a k-th cosine exactly on thr_eff + eps8"""
    a, b, e = launches["anchored"], launches["budget"], launches["equality"]
    ra, rb = S.check_launch(a, a.opts), S.check_launch(b, b.opts)
    assert ra["anchored"] >= 4 and rb["anchored"] == 0
    assert (a.thr_int[:8].astype(np.float64) * a.unit < -0.1).sum() >= 2
    assert ra["overflow"] >= 1 and (a.pcnt > 256).any() and ra["certified"] >= 3 and ra["uncertified"] >= 1
    assert rb["uncertified"] > ra["uncertified"]
    assert a.planted["one_eps"] is True and FakeLaunch("anchored", "one_eps_cut").planted["one_eps"] is False
    assert e.planted["equality"] is True and a.planted["sample_above_found"] is True


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_checker_names_the_stage_of_a_seeded_fault(fault):
    config, prop = FAULTS[fault]
    f = FakeLaunch(config, fault)
    with pytest.raises(S.PropertyError) as e:
        S.check_launch(f, f.opts, final=f.final, stats=f.stats)
    assert e.value.prop == prop, str(e.value)


def test_parent_thr_eff_formula_is_the_seeded_fault():
    """t * unit * (1 + 1e-6) + 1e-7 rounds DOWN for t * unit < -0.1: below (t - 1) * unit, the largest estimate of an uncollected row,
    at the operating points the issue names (dim 1024; sqi 100 / 130 / 400; threshold cosine -0.12 / -0.3 / -0.7)"""
    from oracle import rounding as R
    s0 = R.i8_scale_unit(1024)
    for sqi, c in ((100, -0.12), (130, -0.3), (400, -0.7)):
        unit = s0 * s0 * sqi
        t = int(np.ceil(c / unit))
        parent = float(np.float32(t * unit * (1.0 + 1e-6) + 1e-7))
        fixed = float(np.float32(t * unit + abs(t * unit) * 1e-6 + 1e-7))
        assert parent < (t - 1) * unit < t * unit <= fixed <= t * unit + abs(t * unit) * 2e-6 + 2e-7
