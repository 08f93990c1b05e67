"""The certified re-score's protocol loop in C++ (m3pc_amd/csrc/cert_resolve.h: the ONE loop behind the serial, pipelined and
lock-step certified steps) against m3pc_amd/certificate.py:resolve, without a GPU.  tests/cert_resolve_host.cpp drives the loop
with scripted certificates and a fake ops object and prints the trace of ops calls and the record; the same scripts go through
certificate.resolve with a fake ops object here; trace and record must be equal, delta exactly (deviations and deltas are
powers of two, exact as the float the C side reads and as the double Python computes with).  The program is built with the host
compiler under AddressSanitizer + UBSan and run as a stand-alone executable: a report fails the run.

Every scenario takes one of the loop's branches; only GPU sweeps reached the rare ones (window set, every candidate in fp32,
race-list overflow, delta growth) before."""
import os
import subprocess
import types

import pytest

from m3pc_amd import certificate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D7, D5, D10 = 2.0 ** -7, 2.0 ** -5, 2.0 ** -10  # delta going in; a deviation above delta / 1.5; one below

# name: (N, kmax, rmax, n_done, r_done, delta, grow, reads [(deviation, need, need_race)])
BASE = (625, 32, 32, 6, 2, D7, 1)
SCENARIOS = {
    "certified_at_first_read": BASE + ([(D10, 5, 2)],),
    "extend_score_list": BASE + ([(D10, 20, 2), (D10, 20, 2)],),
    "extend_twice": BASE + ([(D10, 20, 2), (D10, 27, 2), (D10, 27, 2)],),
    "extend_race_list": BASE + ([(D10, 5, 9), (D10, 5, 9)],),
    "extend_both_in_one_turn": BASE + ([(D10, 11, 9), (D10, 11, 9)],),
    "window_set_satisfied": BASE + ([(D10, 100, 2), (D10, 90, 2)],),
    "window_set_still_short": BASE + ([(D10, 100, 2), (D10, 140, 2), (D10, 1, 1)],),
    "need_above_n": BASE + ([(D10, 700, 2), (D10, 1, 1)],),
    "race_overflow": BASE + ([(D10, 5, 40), (D10, 1, 1)],),
    "delta_growth_with_work_left": BASE + ([(D5, 5, 2), (D5, 20, 2), (D5, 20, 2)],),
    "growth_disabled": (625, 32, 32, 6, 2, D7, 0, [(D5, 5, 2)]),
    "n_not_above_n_done": (4, 32, 2, 4, 2, D7, 1, [(D5, 9, 2)]),
    "race_extension_after_window_set": BASE + ([(D10, 100, 2), (D10, 90, 5), (D10, 90, 5)],),
    "delta_growth_after_window_set": BASE + ([(D10, 100, 2), (D5, 90, 2), (D5, 90, 2)],),
    "rmax_zero": (625, 32, 0, 6, 0, D7, 1, [(D10, 20, 0), (D10, 20, 0)]),
}
# the branch each scenario is there for: ops calls its trace must hold, in this order (reads left out)
BRANCH = {
    "certified_at_first_read": [],
    "extend_score_list": ["extend 6 20", "merge_select"],
    "extend_twice": ["extend 6 20", "merge_select", "extend 20 27", "merge_select"],
    "extend_race_list": ["extend_race 2 9", "merge_select"],
    "extend_both_in_one_turn": ["extend 6 11", "extend_race 2 9", "merge_select"],
    "window_set_satisfied": ["window_set 100 0"],
    "window_set_still_short": ["window_set 100 0", "window_set 625 1"],
    "need_above_n": ["window_set 700 0"],
    "race_overflow": ["window_set 625 1"],
    "delta_growth_with_work_left": ["merge_select", "extend 6 20", "merge_select"],
    "growth_disabled": [],
    "n_not_above_n_done": [],
    "race_extension_after_window_set": ["window_set 100 0", "extend_race 2 5", "merge_select"],
    "delta_growth_after_window_set": ["window_set 100 0", "merge_select"],
    "rmax_zero": ["extend 6 20", "merge_select"],
}
# What the eval certificate relies on: the loop entered again on the SAME state after an extension (name: scenario, then the
# n_done the turn between the entries extends to; 0: none).  certificate.resolve has no second entry: the traces are written out.
REENTRY = {
    "reentry_keeps_need_first": (BASE + ([(D10, 5, 2), (D10, 20, 2), (D10, 20, 2)],), 12),
    "reentry_keeps_saturated": (BASE + ([(D10, 100, 2), (D10, 90, 2), (D10, 120, 2), (D10, 1, 1)],), 0),
}


def _g(x):
    return "%.17g" % x


class _Ops:
    """certificate.py's ops, faked: pops the next scripted read and logs every call in the format of cert_resolve_host.cpp."""

    def __init__(self, N, rmax, n_done, r_done, reads):
        self.N, self.rmax, self.n_done, self.r_done = N, rmax, n_done, r_done
        self.reads, self.next, self.everything, self.trace = reads, 0, False, []

    def read(self):
        # (four_only as the C loop hints it: fp32 scores for every candidate, or no race list)
        self.trace.append("read %d" % (self.everything or self.rmax == 0))
        dev, need, race = self.reads[self.next]
        self.next += 1
        return [self.next / 8.0, dev, float(need), self.next / 16.0, float(race), 0.0, 0.0]

    def extend(self, lo, hi):
        self.trace.append("extend %d %d" % (lo, hi))
        self.n_done = hi

    def extend_race(self, lo, hi):
        self.trace.append("extend_race %d %d" % (lo, hi))
        self.r_done = hi

    def window_set(self, need, delta, everything=False):
        self.trace.append("window_set %d %d %s" % (need, everything, _g(delta)))
        self.n_done = self.N if everything else min(need, self.N)
        self.everything = self.everything or everything or self.n_done >= self.N
        return self.n_done

    def merge_select(self, n, r, delta):
        assert (n, r) == (self.n_done, self.r_done)
        self.trace.append("merge_select %d %d %s" % (n, r, _g(delta)))


def _python(N, kmax, rmax, n_done, r_done, delta, grow, reads):
    planner = types.SimpleNamespace(_delta_fixed=None if grow else delta, delta_grown=0, _warned_saturated=True, rescore_max=kmax)
    ops = _Ops(N, rmax, n_done, r_done, reads)
    rec = certificate.resolve(planner, N, kmax, rmax, n_done, r_done, delta, ops)
    record = dict(rc=0, n_rescored=rec["n_rescored"], n_race=rec["n_race"], need_first=rec["n_in_window"], need_race_first=rec["need_race"],
                  saturated=int(rec["saturated"]), everything=int(ops.everything), certified=int(rec["certified"]), rounds=0,
                  delta=rec["delta"], shift=rec["shift"], deviation=rec["deviation"], margin=rec["min_margin_outside"],
                  reads_left=len(reads) - ops.next)
    return ops.trace, record


def _script(name, sc, ext=None):
    N, kmax, rmax, n_done, r_done, delta, grow, reads = sc
    head = "%s %d %d %d %d %d %s %d %d %d" % (name, N, kmax, rmax, n_done, r_done, _g(delta), grow, len(reads), 1 if ext is None else 2)
    return "\n".join([head] + ["%s %d %d" % (_g(d), n, r) for d, n, r in reads] + ([] if ext is None else [str(ext)])) + "\n"


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """{scenario: (trace, record)} and the trailing lines of ONE run of the sanitized stand-alone program over every script."""
    exe = str(tmp_path_factory.mktemp("cert_resolve") / "cert_resolve_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "m3pc_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cert_resolve_host.cpp"), "-o", exe])
    text = "".join(_script(n, sc) for n, sc in SCENARIOS.items()) + "".join(_script(n, sc, ext) for n, (sc, ext) in REENTRY.items())
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", f"the sanitized program reported:\n{run.stderr}"
    out, tail, cur = {}, [], None
    for line in run.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word == "scenario":
            cur = rest
            out[cur] = ([], None)
        elif word == "record":
            rec = {k: (float(v) if k in ("delta", "shift", "deviation", "margin") else int(v)) for k, v in (f.split("=") for f in rest.split())}
            out[cur] = (out[cur][0], rec)
            cur = None
        elif cur is not None:
            out[cur][0].append(line)
        else:
            tail.append(line)
    return out, tail


def test_every_scenario_ran(native):
    assert list(native[0]) == list(SCENARIOS) + list(REENTRY)
    assert set(BRANCH) == set(SCENARIOS)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_loop_matches_the_python_protocol(native, name):
    trace_c, rec_c = native[0][name]
    trace_py, rec_py = _python(*SCENARIOS[name])
    assert trace_c == trace_py
    assert rec_c == rec_py  # (delta, shift, deviation, margin: exact)
    assert rec_c["reads_left"] == 0 and rec_c["certified"] == 1
    # the scenario takes the branch it is named after
    calls = [" ".join(t.split()[:3]) if t.startswith("window_set") else t for t in trace_c if not t.startswith("read")]
    calls = ["merge_select" if t.startswith("merge_select") else t for t in calls]
    assert calls == BRANCH[name]
    assert len([t for t in trace_c if t.startswith("read")]) == len(SCENARIOS[name][7])


def test_branch_details(native):
    out = native[0]
    assert out["growth_disabled"][1]["delta"] == D7 and out["growth_disabled"][0] == ["read 0"]
    assert out["n_not_above_n_done"][1]["delta"] == 1.5 * D5 and out["n_not_above_n_done"][0] == ["read 0"]
    assert out["delta_growth_with_work_left"][0][1] == "merge_select 6 2 " + _g(1.5 * D5)
    assert out["delta_growth_after_window_set"][0][-2] == "merge_select 100 2 " + _g(1.5 * D5)
    assert out["need_above_n"][1]["everything"] == 1 and out["need_above_n"][1]["n_rescored"] == 625
    assert out["need_above_n"][0][-1] == "read 1"  # (behind fp32 scores for every candidate the merge wrote four statistics)
    assert out["race_overflow"][1]["saturated"] == 1 and out["race_overflow"][1]["everything"] == 1
    assert out["window_set_satisfied"][1]["saturated"] == 1 and out["window_set_satisfied"][1]["everything"] == 0
    assert all(t == "read 1" for t in out["rmax_zero"][0] if t.startswith("read"))


def test_second_entry_keeps_need_first(native):
    trace, rec = native[0]["reentry_keeps_need_first"]
    d = _g(D7)
    assert trace == ["read 0", "extend 6 12", f"merge_select 12 2 {d}", "enter", "read 0", "extend 12 20", f"merge_select 20 2 {d}", "read 0"]
    assert (rec["need_first"], rec["need_race_first"], rec["n_rescored"], rec["certified"], rec["reads_left"]) == (5, 2, 20, 1, 0)
    assert (rec["shift"], rec["margin"]) == (3 / 8, 3 / 16)  # the LAST read's


def test_second_entry_keeps_saturated(native):
    trace, rec = native[0]["reentry_keeps_saturated"]
    d = _g(D7)
    # saturated came in with the state: what asks for more goes straight to every candidate in fp32, not to a second window set
    assert trace == ["read 0", f"window_set 100 0 {d}", "read 0", "enter", "read 0", f"window_set 625 1 {d}", "read 1"]
    assert (rec["saturated"], rec["everything"], rec["n_rescored"], rec["need_first"], rec["certified"], rec["reads_left"]) == (1, 1, 625, 100, 1, 0)


def test_fp32_record_and_cert_delta(native):
    tail = native[1]
    assert tail[0] == "fp32 n_rescored=625 everything=1 certified=1 saturated=0 rounds=0 delta=0"
    # max(factor x deviation, 1e-6 x scale, 1e-30), rounded once to float
    import numpy as np
    want = [np.float32(0.25), np.float32(1e-6 * 8.0), np.float32(1e-30)]
    assert [float(v) for v in tail[1].split()[1:]] == [float(w) for w in want]
