"""cert_resolve_eval (m3pc_amd/csrc/cert_resolve.h: the protocol loop with the eval_action certificate behind it -- the ONE function
behind m3pc_plan_step_certified_eval, _eval_end and a window of m3pc_plan_steps_certified_eval) without a GPU.
tests/cert_resolve_eval_host.cpp drives it with scripted certificates, a scripted bound kernel (bound(n') = b0 2^-(n' - n)) and fake
ops that also play the pipelined step's bound launched in advance; the trace of ops calls and both records are compared with what
the header's contract says, written out here.  Built with the host compiler under AddressSanitizer + UBSan and run as a stand-alone
executable: a report fails the run.

An eval_read line is ``eval_read n_listed r_done n_done delta taken``: taken = 1 when the block launched in advance was used."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D7, D5, D10 = 2.0 ** -7, 2.0 ** -5, 2.0 ** -10  # delta going in; a deviation above delta / 1.5; one below
B, T3, T17 = 2.0 ** -3, 2.0 ** -3, 2.0 ** -17   # the bound at the first n_done; a tolerance it meets; one 14 more entries meet
INF = float("inf")


def _g(x):
    return "%.17g" % x


d, g = _g(D7), _g(1.5 * D5)
BASE = (625, 32, 32, 6, 2, D7, 1)
# name: (N, kmax, rmax, n_done, r_done, delta, grow, eval_tol, reads [(deviation, need, need_race)], bounds [b0], trace, records)
SCENARIOS = {
    # certified at the first bound, the block launched in advance valid
    "spec_valid_certified": BASE + (T3, [(D10, 5, 2)], [B], ["read 0", f"eval_read 32 2 6 {d} 1"],
                                    dict(n_rescored=6, merges=0, eval_bound=B, need_eval_first=6, n_eval=0, eval_rounds=1, everything=0)),
    # ... invalid because a certificate asked for an extension: the dropped launch is no eval round
    "spec_invalid_extension": BASE + (T3, [(D10, 20, 2), (D10, 20, 2)], [B],
                                      ["read 0", "extend 6 20", f"merge_select 20 2 {d}", "read 0", f"eval_read 32 2 20 {d} 0"],
                                      dict(n_rescored=20, merges=1, eval_bound=B, need_eval_first=20, n_eval=0, eval_rounds=1, everything=0)),
    # ... invalid because delta grew
    "spec_invalid_delta_grew": BASE + (T3, [(D5, 5, 2), (D5, 5, 2)], [B], ["read 0", f"merge_select 6 2 {g}", "read 0", f"eval_read 32 2 6 {g} 0"],
                                       dict(n_rescored=6, merges=1, delta=1.5 * D5, eval_bound=B, need_eval_first=6, n_eval=0, eval_rounds=1,
                                            everything=0)),
    "one_eval_extension": BASE + (T17, [(D10, 5, 2), (D10, 5, 2)], [B, T17],
                                  ["read 0", f"eval_read 32 2 6 {d} 1", "extend 6 20", f"merge_select 20 2 {d}", "read 0", f"eval_read 32 2 20 {d} 0"],
                                  dict(n_rescored=20, merges=1, eval_bound=T17, need_eval_first=20, n_eval=14, eval_rounds=2, everything=0)),
    # an eval extension, then the certificates of the longer list raise delta and ask for more, then the bound asks again
    "eval_extension_delta_growth_further_need": BASE + (
        T17, [(D10, 5, 2), (D5, 5, 2), (D5, 25, 2), (D5, 25, 2), (D5, 25, 2)], [B, 2.0 ** -14, T17],
        ["read 0", f"eval_read 32 2 6 {d} 1", "extend 6 20", f"merge_select 20 2 {d}", "read 0", f"merge_select 20 2 {g}", "read 0",
         "extend 20 25", f"merge_select 25 2 {g}", "read 0", f"eval_read 32 2 25 {g} 0", "extend 25 28", f"merge_select 28 2 {g}", "read 0",
         f"eval_read 32 2 28 {g} 0"],
        dict(n_rescored=28, merges=4, delta=1.5 * D5, eval_bound=T17, need_eval_first=20, n_eval=17, eval_rounds=3, everything=0)),
    # the list cannot reach the tolerance: every candidate in fp32, bound 0
    "need_eval_beyond_the_list": BASE + (2.0 ** -40, [(D10, 5, 2), (D10, 1, 1)], [B],
                                         ["read 0", f"eval_read 32 2 6 {d} 1", f"window_set 625 1 {d}", "read 1"],
                                         dict(n_rescored=625, merges=1, eval_bound=0.0, need_eval_first=625, n_eval=0, eval_rounds=1, everything=1)),
    # behind a window set the list is wholly re-scored: n_listed = n_done
    "behind_window_set_within_tol": BASE + (T3, [(D10, 100, 2), (D10, 90, 2)], [B],
                                            ["read 0", f"window_set 100 0 {d}", "read 0", f"eval_read 100 2 100 {d} 0"],
                                            dict(n_rescored=100, merges=1, saturated=1, eval_bound=B, need_eval_first=100, n_eval=0, eval_rounds=1,
                                                 everything=0)),
    "behind_window_set_beyond_tol": BASE + (T17, [(D10, 100, 2), (D10, 90, 2), (D10, 1, 1)], [B],
                                            ["read 0", f"window_set 100 0 {d}", "read 0", f"eval_read 100 2 100 {d} 0", f"window_set 625 1 {d}", "read 1"],
                                            dict(n_rescored=625, merges=2, saturated=1, eval_bound=0.0, need_eval_first=625, n_eval=0, eval_rounds=1,
                                                 everything=1)),
    "rmax_zero": (625, 32, 0, 6, 0, D7, 1, T3, [(D10, 5, 0)], [B], ["read 1", f"eval_read 32 0 6 {d} 1"],
                  dict(n_rescored=6, n_race=0, merges=0, eval_bound=B, need_eval_first=6, n_eval=0, eval_rounds=1, everything=0)),
    # report only: the bound is read once, nothing is extended whatever it is
    "eval_tol_inf": BASE + (INF, [(D10, 5, 2)], [2.0 ** 10], ["read 0", f"eval_read 32 2 6 {d} 1"],
                            dict(n_rescored=6, merges=0, eval_bound=2.0 ** 10, need_eval_first=6, n_eval=0, eval_rounds=1, everything=0)),
    # every candidate is re-scored already: no bound is asked for
    "every_candidate_rescored": (4, 32, 2, 4, 2, D7, 1, T3, [(D5, 9, 2)], [], ["read 0"],
                                 dict(n_rescored=4, merges=0, delta=1.5 * D5, eval_bound=0.0, need_eval_first=0, n_eval=0, eval_rounds=0,
                                      everything=0)),
}


def _script(name, sc):
    N, kmax, rmax, n_done, r_done, delta, grow, tol, reads, bounds = sc[:10]
    head = "%s %d %d %d %d %d %s %d %s %d %d" % (name, N, kmax, rmax, n_done, r_done, _g(delta), grow, "inf" if tol == INF else _g(tol),
                                                len(reads), len(bounds))
    return "\n".join([head] + ["%s %d %d" % (_g(dv), n, r) for dv, n, r in reads] + [_g(b) for b in bounds]) + "\n"


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """{scenario: (trace, record)} of ONE run of the sanitized stand-alone program over every script."""
    exe = str(tmp_path_factory.mktemp("cert_resolve_eval") / "cert_resolve_eval_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "m3pc_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cert_resolve_eval_host.cpp"), "-o", exe])
    text = "".join(_script(n, sc) for n, sc in SCENARIOS.items())
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", f"the sanitized program reported:\n{run.stderr}"
    out, cur = {}, None
    for line in run.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word == "scenario":
            cur = rest
            out[cur] = ([], None)
        elif word == "record":
            rec = {k: (float(v) if k in ("delta", "shift", "eval_bound") else int(v)) for k, v in (f.split("=") for f in rest.split())}
            out[cur] = (out[cur][0], rec)
            cur = None
        else:
            assert cur is not None, line
            out[cur][0].append(line)
    return out


def test_every_scenario_ran(native):
    assert list(native) == list(SCENARIOS)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_trace_and_records(native, name):
    sc = SCENARIOS[name]
    trace, rec = native[name]
    assert trace == sc[10]
    want = dict(rc=0, n_race=2, saturated=0, certified=1, delta=D7, reads_left=0, bounds_left=0, eval_certified=1,
                need_first=sc[8][0][1], need_race_first=sc[8][0][2], shift=len(sc[8]) / 8.0)
    want.update(sc[11])
    assert rec == want
    # eval_rounds counts the bounds the loop read, and nothing else
    assert rec["eval_rounds"] == len([t for t in trace if t.startswith("eval_read")]) == len(sc[9])


def test_speculation_rule(native):
    """The block launched in advance is taken exactly at a first eval_read that no merge precedes."""
    for name, (trace, _) in native.items():
        seen_merge, first = False, True
        for t in trace:
            if t.startswith(("merge_select", "window_set")):
                seen_merge = True
            if t.startswith("eval_read"):
                assert int(t.split()[-1]) == int(first and not seen_merge), (name, t)
                first = False
