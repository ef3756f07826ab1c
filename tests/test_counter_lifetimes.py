"""Who holds the device copy of the per-node path-position tables (counters.hip, Counters::d_*): report coverage, shared reads,
equivalence classes and assigned coverage read ONE copy, uploaded when the first of them comes on and released when the last goes off.
The counters are switched on and off in every order that hands the copy from one holder to another, on one ctx, with one batch between
the steps; after each step every counter that is on equals the CPU oracle's sum over the batches fed since it last came on, and every
counter that is off refuses its export.

The index and the batches are those of test_counter_edges.py (`plain` and `plain2`, 6 000 reads each: fast-path, slow-path and
multi-word sets, asserted there on the CPU by test_inputs_reach_every_edge); the expectations come from its _Want / _Total / _check,
from table_of_alns / _dev_table of test_calls.py for assigned coverage and from _PWant of test_paired.py in paired mode -- never from a
second device run."""
import pytest

import test_calls as calls
import test_counter_edges as ce
import test_paired as tp
from groot_amd import host
from test_coverage import _stage

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    """(the index of the seven graphs, plain, plain2)"""
    index, batches = ce._build_case(tmp_path_factory.mktemp("counter_lifetimes"))
    assert [b.name for b in batches] == ["plain", "clip", "plain2"] and batches[0].n == batches[2].n == 6000
    return index, batches[0], batches[2]


_FLAGS = {"cov": dict(cov=True, sh=False, ec=False), "sh": dict(cov=False, sh=True, ec=False), "ec": dict(cov=False, sh=False, ec=True)}


class _Script:
    """switches counters, feeds batches, and knows which batches every counter that is on has seen since it came on"""

    def __init__(self, al, index, paired):
        self.al, self.index, self.paired, self.since, self.first = al, index, paired, {}, 0
        self.switch = {"cov": al.coverage_enable, "sh": al.shared_enable, "ec": al.ec_enable, "acov": al.acov_enable}
        self.export = {"cov": al.coverage, "sh": al.shared, "ec": al.ecs, "acov": al.acov}

    def on(self, name):
        assert name not in self.since
        self.switch[name](True)
        self.since[name] = []
        if name == "acov":                                   # (brings equivalence classes on)
            self.since.setdefault("ec", [])

    def off(self, name):
        self.switch[name](False)
        del self.since[name]
        if name == "ec":                                     # (takes assigned coverage with it)
            self.since.pop("acov", None)

    def feed(self, b):
        self.first = ce._feed(self.al, [b], self.first)
        for seen in self.since.values():
            seen.append(b)

    def verify(self):
        al, index = self.al, self.index
        want = (lambda b: tp._pwant(index, b)) if self.paired else (lambda b: b.want(index))
        for name, flags in _FLAGS.items():
            if name in self.since:
                ce._check(al, index, [want(b) for b in self.since[name]], **flags)
        if "acov" in self.since:
            calls._check(al, index, self.since["acov"])
        if self.paired and "sh" in self.since:
            st = al.pairs_stats()
            print("pairs", st)
            assert st["joined"] + 2 * st["split"] + st["single"] == al.shared_stats()["reads"] > 0
        for name, export in self.export.items():
            if name not in self.since:
                with pytest.raises(host.GrootError):
                    export()
        assert al.acov_stats()["slots"] == 0 or "acov" in self.since


@pytest.mark.parametrize("mode", ["default", "eight_slots", "paired"])
def test_the_shared_tables_pass_from_holder_to_holder(case, hip_lib, monkeypatch, mode):
    """default: the tables of the shipped sizes; eight_slots: GROOT_TEST_EC_SLOTS=8 GROOT_TEST_ACOV_SLOTS=8, both run-wide tables grow
    and swap their buffers while coverage holds the copy too; paired: pairing on, equivalence classes where assigned coverage (which
    refuses paired units) stands in the other two"""
    index, plain, plain2 = case
    paired = mode == "paired"
    _stage(monkeypatch, "path_first")
    if mode == "eight_slots":
        monkeypatch.setenv("GROOT_TEST_EC_SLOTS", "8")
        monkeypatch.setenv("GROOT_TEST_ACOV_SLOTS", "8")
    al = ce._open(index, [plain, plain2], cov=False, sh=False, ec=False)
    try:
        s = _Script(al, index, paired)
        if paired:
            al.pairs_enable()
        s.verify()                                           # nothing is on: every export refuses
        # 1. coverage on -> assigned coverage on (brings equivalence classes on) -> coverage off
        s.on("cov")
        s.feed(plain)
        s.verify()
        if paired:
            with pytest.raises(host.GrootError):
                al.acov_enable()
            s.on("ec")
        else:
            s.on("acov")
            assert al.ec_stats()["reads"] == 0
        s.feed(plain2)
        s.verify()
        if mode == "eight_slots":
            assert al.ec_stats()["grows"] >= 1 and al.acov_stats()["grows"] >= 1
        s.off("cov")
        s.feed(plain)
        s.verify()
        # 2. shared reads on -> equivalence classes off (takes assigned coverage with it) -> only shared reads left
        s.on("sh")
        s.feed(plain2)
        s.verify()
        s.off("ec")
        assert sorted(s.since) == ["sh"]
        s.feed(plain)
        s.verify()
        # 3. shared reads off: all four are off, a batch runs and launches nothing for them -> coverage on again
        s.off("sh")
        assert not s.since
        launches = al.acov_stats()["launches"]
        assert paired or launches > 0
        s.feed(plain2)
        assert al.acov_stats()["launches"] == launches
        s.verify()
        s.on("cov")
        s.feed(plain)
        s.verify()
        assert [b.name for b in s.since["cov"]] == ["plain"]
    finally:
        al.close()
