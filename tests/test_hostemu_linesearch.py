"""CPU tier: the decision code of the filter line search (linesearch_begin / linesearch_decide of bipedal_control_amd/csrc/kernels/linesearch.h, compiled
by g++ through the lane emulation) against a plain restatement in Python floats (tests/linesearch_cases.filter_linesearch, written from the oracle).

The numbers are synthetic and exactly representable (tests/linesearch_cases.table_cases): a comparison that sits ON its threshold is the same comparison
in both implementations, and every sum is exact, so every field is compared for equality.  Each case runs with the deciding workgroup's three lane
counts: 64 (reference kernels), 256 (k_ls_decide) and 512 (k_ls_tail)."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import linesearch_cases as lc

dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
CASES = lc.table_cases()
LANES = (64, 256, 512)


def run_emulation(lib, case, lanes):
    """The entry point emu_linesearch of tests/hostemu/hostemu.cpp on a table case: the same dict as filter_linesearch returns."""
    f = lambda a: np.ascontiguousarray(a, float).copy()
    st = case["settings"]
    x, u = f(case["x"]), f(case["u"])
    tables = f(np.concatenate(case["trial_tables"])) if case["trial_tables"] else np.zeros(1)
    state = np.array([-5, case["active"], case["iterations"], case["remaining"]], np.int32)
    stats, out = np.full(lc.STATS, lc.UNTOUCHED), np.zeros(4)
    d = lambda a: a.ctypes.data_as(dp)
    keep = [f(case[k]) for k in ("node_perf", "x0", "dx", "du", "summary")] + [np.array([float(st[k]) for k in lc.SETTING_ORDER])]
    lib.emu_linesearch.restype = C.c_int
    rounds = lib.emu_linesearch(case["nx"] - 12, lanes, case["n_nodes"], len(case["trial_tables"]), d(keep[0]), d(tables), d(keep[1]), d(x), d(u), d(keep[2]),
                                d(keep[3]), d(keep[4]), d(keep[5]), state.ctypes.data_as(ip), d(stats), d(out))
    assert rounds >= 0
    return dict(stats=list(stats), alpha=float(out[0]), base=list(out[1:4]), done=int(state[0]), active=int(state[1]), iterations=int(state[2]),
                remaining=int(state[3]), rounds=rounds, x=list(x), u=list(u))


@pytest.fixture(scope="module")
def results(hostemu_lib):
    return {(name, lanes): run_emulation(hostemu_lib, case, lanes) for name, (case, _) in CASES.items() for lanes in LANES}


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_field_equals_the_restatement(results, name, lanes):
    case, _ = CASES[name]
    got, ref = results[name, lanes], lc.filter_linesearch(case)
    for key in ("done", "active", "iterations", "remaining", "rounds", "alpha"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    for i, (a, b) in enumerate(zip(got["stats"], ref["stats"])):
        assert a == b, ("stats", i, a, b)
    for i, (a, b) in enumerate(zip(got["base"], ref["base"])):
        assert abs(a - b) <= 1e-15 * abs(b), ("base", i, a, b)
    assert got["x"] == ref["x"] and got["u"] == ref["u"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_case_shows_what_it_exists_for(results, name):
    """The expected outcome of each case, worked out by hand in table_cases, on the restatement AND on the emulated kernel code."""
    case, want = CASES[name]
    for who, r in [("restatement", lc.filter_linesearch(case))] + [(lanes, results[name, lanes]) for lanes in LANES]:
        s = r["stats"]
        seen = dict(status=s[2], step=s[9], rounds=r["rounds"], active=r["active"], iterations=r["iterations"], remaining=r["remaining"], done=r["done"])
        for key, value in want.items():
            if key == "untouched":
                assert r["x"] == list(case["x"]) and r["u"] == list(case["u"]), who
            elif key == "record_untouched":
                assert all(v == lc.UNTOUCHED for v in s), who
            else:
                assert seen[key] == value, (who, key, seen[key], value)
        if "status" in want:
            assert r["done"] == 1 and all(v == lc.UNTOUCHED for v in s[13:]), who        # ended, and nothing written past the record's 13 fields
            assert s[1] == r["iterations"] == case["iterations"] + 1
            if want["status"] != 0:
                assert s[9] == 0.0 and s[11] == 0.0 and s[12] == 0.0 and s[6:9] == s[3:6], who                # no step: the record repeats the linearisation
                assert r["x"] == list(case["x"]) and r["u"] == list(case["u"]), who


@pytest.mark.parametrize("n", lc.NODE_COUNTS)
def test_node_sums_and_the_initial_state_mismatch(results, n):
    """The three sums against math.fsum to 1e-15 relative at node counts around the lane counts (below nx the summing lanes are chosen by
    max(n_nodes, nx)), and the measured state's mismatch counted exactly once, in the linearisation and in every trial."""
    case, _ = CASES["nodes_%d" % n]
    nx = case["nx"]
    base_mismatch = math.fsum(float(v) ** 2 for v in case["x0"] - case["x"][:nx])
    half_mismatch = math.fsum(float(v) ** 2 for v in case["x0"] - (case["x"][:nx] + 0.5 * case["dx"][:nx]))
    assert base_mismatch > 1.0 / 1024 and half_mismatch > 1.0 / 1024 and half_mismatch != base_mismatch
    want = [8.0, 12.0 + base_mismatch, 4.0, 4.0, 0.5 + half_mismatch, 0.5]
    for lanes in LANES:
        s = results["nodes_%d" % n, lanes]["stats"]
        for got, ref in zip(s[3:9], want):
            assert abs(got - ref) <= 1e-15 * abs(ref), (lanes, got, ref)
        assert s[0] == float(n)


def test_a_search_out_of_tables_is_still_open(hostemu_lib):
    """The entry point neither spins nor decides without a trial: with fewer tables than the search needs it returns with the search open."""
    case, _ = CASES["nan_merit"]
    short = dict(case, trial_tables=case["trial_tables"][:5])
    got, ref = run_emulation(hostemu_lib, short, 64), lc.filter_linesearch(short)
    assert got["done"] == ref["done"] == 0 and got["rounds"] == 5 and got["alpha"] == ref["alpha"] == 2.0 ** -5 and got["remaining"] == ref["remaining"] == 1
    assert all(v == lc.UNTOUCHED for v in got["stats"])


def test_stand_alone_driver_under_address_and_undefined_sanitizers(tmp_path):
    """The same table through tests/hostemu/linesearch_driver.cpp, a program of its own built with -fsanitize=address,undefined (the sanitised code is
    never loaded into Python): every case at every lane count in one run, no report from either sanitizer, and the same results as the restatement."""
    import os
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
    exe = str(tmp_path / "linesearch_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DBPMPC_HOST_EMULATION", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(here, "linesearch_driver.cpp")])
    order, lines = [], []
    for name, (case, _) in sorted(CASES.items()):
        for lanes in LANES:
            order.append((name, lanes))
            head = [case["nx"] - 12, lanes, case["n_nodes"], len(case["trial_tables"]), case["active"], case["iterations"], case["remaining"]]
            arrays = [case["node_perf"]] + list(case["trial_tables"]) + [case[k] for k in ("x0", "x", "u", "dx", "du", "summary")]
            arrays.append([float(case["settings"][k]) for k in lc.SETTING_ORDER])
            lines.append(" ".join([str(v) for v in head] + [repr(float(v)) for a in arrays for v in a]))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    out = run.stdout.strip().split("\n")
    assert len(out) == len(order)
    for (name, lanes), line in zip(order, out):
        case, _ = CASES[name]
        ref = lc.filter_linesearch(case)
        v = line.split()
        got_int, got = [int(t) for t in v[:5]], [float(t) for t in v[5:]]
        assert got_int == [ref["rounds"], ref["done"], ref["active"], ref["iterations"], ref["remaining"]], (name, lanes)
        assert got[0] == ref["alpha"] and got[1:4] == ref["base"] and got[4:4 + lc.STATS] == ref["stats"], (name, lanes)
        assert got[4 + lc.STATS:] == ref["x"] + ref["u"], (name, lanes)
