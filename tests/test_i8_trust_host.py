"""The int8 residual's host-only decisions (csrc/i8_trust.h) -- no GPU: the size thresholds from which its products pay, and the
guard's trust record (first verdict, later batches folded in, reset by a new kernel matrix).  The header is driven by a stand-alone
program under the address and undefined-behaviour sanitizers (tests/sanitize/i8_trust_main.cpp), as test_trsm_order_host.py does
with the persistent solves' scheduler."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the runtimes are linked INTO the program: it does not depend on what else the machine loads into its processes, or in which order
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
THR = 1e-5  # kI8FloorThr; the header takes the threshold as an argument


def _static_runtime(name):
    p = subprocess.check_output(["gcc", "-print-file-name=" + name]).decode().strip()
    return p if os.path.isabs(p) else None


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if _static_runtime("libasan.a") is None or _static_runtime("libubsan.a") is None:
        pytest.skip("no static sanitizer runtime (libasan.a, libubsan.a)")
    tmp = tmp_path_factory.mktemp("i8_trust")
    out = str(tmp / "i8_trust_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "i8_trust_main.cpp"), "-o", out],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0 and build.stderr == "", build.stderr[-4000:]  # a build that fails, or warns, is a failure
    return out, tmp


def _run(exe, name, commands):
    """Runs the commands in order on one trust record; per command (checked, distrusted, pending, floor_ratio, result)."""
    prog, tmp = exe
    script = str(tmp / (name + ".txt"))
    with open(script, "w") as f:
        f.write("\n".join(commands) + "\n")
    run = subprocess.run([prog, script], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    rows = [line.split() for line in run.stdout.strip().split("\n")]
    assert len(rows) == len(commands)
    return [(r[0] == "1", r[1] == "1", r[2] == "1", float(r[3]), int(r[4])) for r in rows]


def test_a_new_kernel_clears_checked_distrusted_and_pending(exe):
    rows = _run(exe, "new", ["first 1e-3 %r" % THR, "pending", "new"])
    assert rows[0][:3] == (True, True, False) and rows[0][4] == 1
    assert rows[1][:3] == (True, True, True)
    assert rows[2][:3] == (False, False, False)
    assert _run(exe, "fresh", ["new"])[0] == (False, False, False, -1.0, 0)   # a record nobody has touched: trusted, nothing seen


def test_first_verdict_below_at_and_above_the_threshold(exe):
    below = _run(exe, "below", ["first 4e-8 %r" % THR])[0]
    assert below == (True, False, False, 4e-8, 0)                    # floor_ratio is the ratio itself; no redo
    at = _run(exe, "at", ["first %r %r" % (THR, THR)])[0]
    assert at == (True, False, False, THR, 0)                        # equal to the threshold is trusted
    above = _run(exe, "above", ["first %r %r" % (math.nextafter(THR, 1.0), THR)])[0]
    assert above == (True, True, False, math.nextafter(THR, 1.0), 1)  # distrusted: form the covariance again
    # the first verdict SETS floor_ratio, also to less than a previous fit's maximum (new_kernel leaves the value alone)
    rows = _run(exe, "lower", ["first 3e-6 %r" % THR, "new", "first 1e-7 %r" % THR])
    assert rows[1][3] == 3e-6 and rows[2] == (True, False, False, 1e-7, 0)


def test_first_verdict_with_threshold_zero_distrusts_a_positive_ratio(exe):
    assert _run(exe, "zero", ["first 4e-8 0"])[0] == (True, True, False, 4e-8, 1)
    assert _run(exe, "zero0", ["first 0 0"])[0] == (True, False, False, 0.0, 0)


def test_fold_keeps_the_maximum_and_clears_pending(exe):
    rows = _run(exe, "fold", ["first 2e-7 %r" % THR, "pending", "fold 5e-7 %r" % THR, "pending", "fold 1e-7 %r" % THR, "fold %r %r" % (THR, THR)])
    assert rows[1][2] and not rows[2][2] and not rows[4][2]        # pending comes down with every fold
    assert [r[3] for r in rows] == [2e-7, 2e-7, 5e-7, 5e-7, 5e-7, THR]  # never lowered
    assert not any(r[1] for r in rows)                               # all at or below the threshold: trusted throughout
    assert all(r[0] for r in rows)                                   # fold leaves `checked` alone


def test_fold_of_a_nan_ratio_distrusts(exe):
    rows = _run(exe, "nan", ["first 2e-7 %r" % THR, "pending", "fold nan %r" % THR])
    assert rows[2][:3] == (True, True, False) and rows[2][3] == 2e-7   # !(nan <= thr); nan > floor_ratio is false


def test_fold_after_distrust_stays_distrusted(exe):
    rows = _run(exe, "sticky", ["first 2e-7 %r" % THR, "fold 1e-3 %r" % THR, "fold 1e-9 %r" % THR, "fold 1e-9 0"])
    assert [r[1] for r in rows] == [False, True, True, True]
    assert [r[3] for r in rows] == [2e-7, 1e-3, 1e-3, 1e-3]
    # ... and so does a first verdict's distrust through later folds below the threshold
    rows = _run(exe, "sticky2", ["first 1e-3 %r" % THR, "fold 1e-9 %r" % THR])
    assert rows[1][:2] == (True, True)


def test_size_thresholds(exe):
    cases = [("coarse", 2047, 256, 0), ("coarse", 2048, 256, 1), ("coarse", 2048, 255, 0), ("coarse", 1 << 40, 255, 0), ("coarse", 2047, 1 << 40, 0),
             ("fine", 4095, 512, 0), ("fine", 4096, 512, 1), ("fine", 4096, 511, 0), ("fine", 1 << 40, 511, 0), ("fine", 4095, 1 << 40, 0),
             ("fine", 2048, 256, 0), ("coarse", 4096, 512, 1)]
    rows = _run(exe, "sizes", ["%s %d %d" % c[:3] for c in cases])
    assert [r[4] for r in rows] == [c[3] for c in cases]
    assert all(r[:4] == (False, False, False, -1.0) for r in rows)   # pure functions: the record is untouched
