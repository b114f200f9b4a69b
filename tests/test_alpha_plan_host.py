"""The deferred alpha solve's host-only decisions (csrc/alpha_plan.h) -- no GPU: what a request asks for, what the next caller has
to run, when the CG may stop early, what info() reports, and what set_alpha / a refit leave behind.  The header is driven by a
stand-alone program under the address and undefined-behaviour sanitizers (tests/sanitize/alpha_plan_main.cpp), as
test_i8_trust_host.py does with the int8 residual's trust record."""
import collections
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the runtimes are linked INTO the program: it does not depend on what else the machine loads into its processes, or in which order
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
ORDER_ONLY, RESUME, FRESH = 0, 1, 2

Plan = collections.namedtuple("Plan", "solved pending partial iters_done max_iters tol iters relres have_event result")


def _static_runtime(name):
    p = subprocess.check_output(["gcc", "-print-file-name=" + name]).decode().strip()
    return p if os.path.isabs(p) else None


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if _static_runtime("libasan.a") is None or _static_runtime("libubsan.a") is None:
        pytest.skip("no static sanitizer runtime (libasan.a, libubsan.a)")
    tmp = tmp_path_factory.mktemp("alpha_plan")
    out = str(tmp / "alpha_plan_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "alpha_plan_main.cpp"), "-o", out],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0 and build.stderr == "", build.stderr[-4000:]  # a build that fails, or warns, is a failure
    return out, tmp


def _run(exe, name, commands):
    """Runs the commands in order on one record; the record (and the command's result) after each."""
    prog, tmp = exe
    script = str(tmp / (name + ".txt"))
    with open(script, "w") as f:
        f.write("\n".join(commands) + "\n")
    run = subprocess.run([prog, script], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    rows = [line.split() for line in run.stdout.strip().split("\n")]
    assert len(rows) == len(commands)
    return [Plan(r[0] == "1", r[1] == "1", r[2] == "1", int(r[3]), int(r[4]), float(r[5]), int(r[6]), float(r[7]), r[8] == "1", int(r[9]))
            for r in rows]


def test_a_record_nobody_has_touched(exe):
    p = _run(exe, "fresh", ["next 0"])[0]
    assert p == Plan(False, False, False, 0, 60, 1e-10, 0, 0.0, False, ORDER_ONLY)


def test_request_defaults_follow_the_factor_shift(exe):
    # max_iters <= 0: (int)min(2000, 60 sqrt(reg_fac / reg)) when reg > 0 and reg_fac > reg, else 60
    cases = [(1.0, 60), (16.0, 240), (256.0, 960), (1000.0, 1897), (65536.0, 2000)]
    rows = _run(exe, "ratio", ["request 0 0 1e-3 %r" % (1e-3 * ratio) for ratio, _ in cases])
    assert [p.max_iters for p in rows] == [want for _, want in cases]
    assert all(p.tol == 1e-10 and p.pending and p.solved and not p.partial for p in rows)
    rows = _run(exe, "noreg", ["request 0 0 0 1e-3", "request -1 -1 0 0", "request 0 0 1e-3 1e-4"])  # reg = 0; a SMALLER factor shift
    assert [p.max_iters for p in rows] == [60, 60, 60] and all(p.tol == 1e-10 for p in rows)
    kept = _run(exe, "kept", ["request 17 1e-7 1e-3 16e-3"])[0]
    assert (kept.max_iters, kept.tol, kept.pending, kept.solved) == (17, 1e-7, True, True)   # explicit values are kept


def test_a_request_supersedes_a_stopped_solve(exe):
    rows = _run(exe, "again", ["request 0 0 1 1", "begin", "note 5 1e-6", "stopped 5", "request 0 0 1 1", "next 1"])
    assert rows[3].partial and not rows[3].pending
    assert rows[4].pending and not rows[4].partial and rows[5].result == FRESH


def test_note_estimates_the_iterations_to_the_requested_tolerance(exe):
    # ceil(it log(tol) / log(rr)) when tol < rr < 1 and it > 0 (none of the ratios of logarithms is an integer)
    for tol, it, rr, want in [(0, 5, 1e-6, 9), (0, 4, 3e-7, 7), (0, 6, 2e-9, 7), (0, 2, 0.5, 67), (1e-8, 5, 1e-6, 7)]:
        p = _run(exe, "est", ["request 0 %r 1 1" % tol, "begin", "note %d %r" % (it, rr)])[2]
        assert (p.iters, p.relres) == (want, rr), (tol, it, rr)
    # otherwise the count itself: converged (rr <= tol), rr = 0, rr >= 1, no iteration
    for it, rr in [(5, 1e-10), (5, 3e-11), (4, 0.0), (3, 1.0), (3, 2.5), (0, 1e-6), (0, 1.0)]:
        p = _run(exe, "plain", ["request 0 0 1 1", "begin", "note %d %r" % (it, rr)])[2]
        assert (p.iters, p.relres) == (it, rr), (it, rr)


def test_iters_and_relres_keep_the_maximum_within_a_run(exe):
    rows = _run(exe, "max", ["request 0 0 1 1", "begin", "note 5 1e-6", "note 4 3e-7", "note 2 0.5", "note 3 1e-11", "begin"])
    assert [(p.iters, p.relres) for p in rows[1:]] == [(0, 0.0), (9, 1e-6), (9, 1e-6), (67, 0.5), (67, 0.5), (0, 0.0)]
    assert not any(p.pending or p.partial for p in rows[1:]) and all(p.solved for p in rows)


def test_next(exe):
    rows = _run(exe, "next", ["request 0 0 1 1", "next 0", "next 1",                       # pending: Fresh, whatever allow_partial is
                              "begin", "note 5 1e-6", "stopped 5", "event", "next 1", "next 0",  # stopped early
                              "begin", "note 9 4e-11", "next 0", "next 1"])                # resumed
    assert [rows[i].result for i in (1, 2)] == [FRESH, FRESH]
    assert rows[5].partial and rows[5].iters_done == 5 and not rows[5].pending
    assert [rows[i].result for i in (7, 8)] == [ORDER_ONLY, RESUME]
    assert not rows[10].partial and (rows[10].iters, rows[10].relres) == (9, 4e-11)        # after Resume and its note: not partial
    assert [rows[i].result for i in (11, 12)] == [ORDER_ONLY, ORDER_ONLY]
    assert all(r == rows[i - 1]._replace(result=r.result) for i, r in enumerate(rows) if i in (1, 2, 7, 8, 11, 12))  # next changes nothing


def test_early_stop_needs_a_correcting_caller_one_column_and_a_tight_tolerance(exe):
    below = math.nextafter(1e-3, 0.0)
    cases = [("0", "1 1 0", 1), ("0", "0 1 0", 0), ("0", "1 2 0", 0), ("0", "1 1 1", 0),   # default tol 1e-10
             ("1e-3", "1 1 0", 0), (repr(below), "1 1 0", 1), ("1e-2", "1 1 0", 0), ("1e-6", "1 1 0", 1)]
    for tol, args, want in cases:
        p = _run(exe, "early", ["request 0 %s 1 1" % tol, "early " + args])[1]
        assert p.result == want, (tol, args)


REACHABLE = {
    "untouched": [],
    "pending": ["request 0 0 1 1"],
    "stopped": ["request 0 0 1 1", "begin", "note 5 1e-6", "stopped 5", "event"],
    "solved": ["request 0 0 1 1", "begin", "note 5 3e-11", "event"],
    "resumed": ["request 0 0 1 1", "begin", "note 5 1e-6", "stopped 5", "event", "begin", "note 9 4e-11", "event"],
    "installed": ["installed 5 1e-11"],
    "pending again": ["request 0 0 1 1", "begin", "note 5 1e-6", "stopped 5", "event", "request 30 1e-9 1 1"],
}


@pytest.mark.parametrize("state", sorted(REACHABLE))
def test_drop_invalidate_and_installed_from_every_reachable_state(exe, state):
    before = (_run(exe, "pre", REACHABLE[state] + ["next 0"]))[-1]._replace(result=0)
    drop = _run(exe, "drop", REACHABLE[state] + ["drop"])[-1]
    assert drop == before._replace(pending=False, partial=False)              # solved, the numbers and the event are kept
    inv = _run(exe, "inv", REACHABLE[state] + ["invalidate"])[-1]
    assert inv == before._replace(pending=False, partial=False, solved=False)
    ins = _run(exe, "ins", REACHABLE[state] + ["installed 5 1e-11", "next 0"])
    assert ins[-2] == before._replace(solved=True, pending=False, partial=False, have_event=False, iters=5, relres=1e-11)
    assert ins[-1].result == ORDER_ONLY
