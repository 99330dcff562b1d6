"""The shortcuts of tests/test_fewer_launches_emulated.py on an MI355X: the periodic first pass in eight stream operations,
the settled top-state pass in two launches, assumed classifications without k_chain_classify, the opening pass of a plan
from nothing without its records -- every plan the oracle's, under BLANCE_SPECULATE=1, 0 and fail."""
import pytest

from blance_amd import hip, synth
from test_fewer_launches_emulated import FIRST_NONSTAY, PERIODIC_CASES, _weighted_config3

pytestmark = pytest.mark.gpu

SPECS = ("1", "0", "fail")


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


def _same(got, want, tag):
    assert (got.digest(), got.iterations, got.n_warnings) == (want.digest(), want.iterations, want.n_warnings), tag


def _plan(fp, spec, monkeypatch, times=1, **kw):
    monkeypatch.setenv("BLANCE_SPECULATE", spec)
    pl = hip.Planner(device_id=0, **kw)
    try:
        return [pl.plan(fp) for _ in range(times)]
    finally:
        pl.close()


def test_config3_reduced_planned_twice(monkeypatch):
    """131,072 x 1,024: every part of the call, twice on one context (the second plan starts from what the first left)."""
    fp = synth.config_flat(3, P=131072, N=1024)
    want = _oracle(fp)
    syncs = {}
    for spec in SPECS:
        for rep, got in enumerate(_plan(fp, spec, monkeypatch, times=2, chain_min_parts=64)):
            _same(got, want, (spec, rep))
        syncs[spec] = got.struct.host_syncs
    assert syncs["1"] == 4, syncs


@pytest.mark.parametrize("which", ["named_weighted", "rebalance"])
def test_settled_pass_refuted_by_its_own_word(monkeypatch, which):
    fp = synth.config3_named_weighted_flat(16384, 512)
    if which == "rebalance":
        fp = synth.config3_rebalance_flat(fp, _oracle(fp))
    want = _oracle(fp)
    for spec in SPECS:
        _same(_plan(fp, spec, monkeypatch, chain_min_parts=64)[0], want, (which, spec))


@pytest.mark.parametrize("where", list(FIRST_NONSTAY))
def test_settled_pass_first_nonstay(monkeypatch, where):
    """4,097 partitions: the one step of the last wave that is in range, or step 0, refutes the assumed pass of sweep 2."""
    fp = _weighted_config3(4097, 256, FIRST_NONSTAY[where](4097))
    want = _oracle(fp)
    for spec in SPECS:
        _same(_plan(fp, spec, monkeypatch, chain_min_parts=64)[0], want, (where, spec))


@pytest.mark.parametrize("name", ["counter_test_fails", "counter_test_fails_everywhere", "missing_nodes", "zones_of_192"])
def test_periodic_regions_judged(monkeypatch, name):
    """Regions that k_period_judge refuses (walked on behind two periods) beside regions that it lets copy."""
    fp = PERIODIC_CASES[name][0]()
    want = _oracle(fp)
    for spec in SPECS:
        _same(_plan(fp, spec, monkeypatch, chain_min_parts=8, periodic=True)[0], want, (name, spec))


def test_config2_reduced(monkeypatch):
    """Both states flat: the primary's opening pass runs ungathered, the replica's excludes and gathers."""
    fp = synth.config_flat(2, P=16384, N=256)
    want = _oracle(fp)
    for spec in SPECS:
        _same(_plan(fp, spec, monkeypatch)[0], want, spec)


def test_plan_from_nothing_odd_sizes(monkeypatch):
    """P no multiple of 1,024 (nor of the nodes), N no multiple of 256."""
    for cfg, P, N in ((2, 50001, 333), (3, 70001, 512)):
        fp = synth.config_flat(cfg, P=P, N=N)
        want = _oracle(fp)
        for spec in SPECS:
            _same(_plan(fp, spec, monkeypatch, chain_min_parts=64)[0], want, (cfg, P, N, spec))
