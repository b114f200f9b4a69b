"""The persistent solves' list scheduler (csrc/trsm_order.cpp) as host code -- no GPU.  Its tables fix how block columns are grouped
per update item and so the bits of every solve: tests/golden/trsm_order_pins.json (scripts/make_trsm_order_pins.py) holds the
tables of the commit recorded there, and both the product library and a sanitized stand-alone build of the same file have to
reproduce them."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from nngp_src_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = json.load(open(os.path.join(ROOT, "tests", "golden", "trsm_order_pins.json")))["cases"]
# the runtimes are linked INTO the program: it does not depend on what else the machine loads into its processes, or in which order
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _digest(items, qof):
    return hashlib.sha256(np.ascontiguousarray(items, "<i4").tobytes() + np.ascontiguousarray(qof, "<i4").tobytes()).hexdigest()


def _queue_major(items, qof, queues):
    """What test_persistent_solve_queues_drain_whoever_draws_from_them (tests/test_host.py) draws from: queue q holds the items with
    queue_of == q in the global start order; the device table is these one behind the other."""
    tables = [np.flatnonzero(qof == q) for q in range(queues)]
    q_off = [0]
    for q in range(8):
        q_off.append(q_off[-1] + (len(tables[q]) if q < queues else 0))
    return items[np.concatenate(tables)], q_off


def test_library_tables_match_the_pinned_ones():
    lib = _lib.load()
    assert len(PINS) == 144
    for pin in PINS:
        (mt, nb, tail, workers), backward, merged, queues = pin["shape"], pin["backward"], pin["merged"], pin["queues"]
        count = ctypes.c_int64(0)
        assert lib.nngp_trsm_ticket_queues(mt, nb, tail, backward, workers, merged, queues, None, None, 0, ctypes.byref(count)) == 0, lib.nngp_last_error()
        assert count.value == pin["count"], pin
        items = np.zeros((count.value, 4), np.int32)
        qof = np.zeros(count.value, np.int32)
        assert lib.nngp_trsm_ticket_queues(mt, nb, tail, backward, workers, merged, queues, items.ctypes.data_as(ctypes.c_void_p),
                                           qof.ctypes.data_as(ctypes.c_void_p), count.value, ctypes.byref(count)) == 0, lib.nngp_last_error()
        assert _digest(items, qof) == pin["sha256"], pin
        if queues == 1:  # nngp_trsm_ticket_order is the same table
            single = np.zeros_like(items)
            assert lib.nngp_trsm_ticket_order(mt, nb, tail, backward, workers, merged, single.ctypes.data_as(ctypes.c_void_p), count.value,
                                              ctypes.byref(count)) == 0, lib.nngp_last_error()
            assert np.array_equal(single, items) and not qof.any()


def _static_runtime(name):
    p = subprocess.check_output(["gcc", "-print-file-name=" + name]).decode().strip()
    return p if os.path.isabs(p) else None


def _run_standalone(tmp, flags):
    """Builds tests/sanitize/trsm_order_main.cpp with csrc/trsm_order.cpp and runs it over the pinned grid, in the environment as
    it is.  A build that fails is a failure, whatever the flags."""
    exe, cases, out = str(tmp / "trsm_order_main"), str(tmp / "cases.txt"), str(tmp / "tables.bin")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall"] + flags + [
        os.path.join(ROOT, "tests", "sanitize", "trsm_order_main.cpp"), os.path.join(ROOT, "nngp-src_amd", "csrc", "trsm_order.cpp"), "-o", exe],
        capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-4000:]
    with open(cases, "w") as f:
        for pin in PINS:
            mt, nb, tail, workers = pin["shape"]
            f.write("%d %d %d %d %d %d %d\n" % (mt, nb, tail, workers, pin["backward"], pin["merged"], pin["queues"]))
    run = subprocess.run([exe, cases, out], capture_output=True, text=True, timeout=600)
    raw = np.fromfile(out, "<i4") if os.path.exists(out) else np.zeros(0, np.int32)
    tables, at = [], 0
    while at < len(raw):
        head, q_off = raw[at:at + 8], raw[at + 8:at + 17]
        n = int(head[7])
        at += 17
        items, qof, tab = raw[at:at + 4 * n].reshape(n, 4), raw[at + 4 * n:at + 5 * n], raw[at + 5 * n:at + 9 * n].reshape(n, 4)
        at += 9 * n
        tables.append((head.tolist(), q_off.tolist(), items, qof, tab))
    return run, tables


@pytest.fixture(scope="module")
def standalone(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("trsm_order")
    have_runtime = _static_runtime("libasan.a") is not None and _static_runtime("libubsan.a") is not None  # decided before the build
    return {"sanitized": _run_standalone(tmp, SAN) if have_runtime else None, "tmp": tmp}


def test_scheduler_runs_clean_under_asan_and_ubsan_and_gives_the_pinned_tables(standalone):
    """The same source file as a program of its own under the address and undefined-behaviour sanitizers (g++, -O1,
    -ffp-contract=off: another compiler at another optimisation level than the library's) over the whole pinned grid."""
    if standalone["sanitized"] is None:
        pytest.skip("no static sanitizer runtime (libasan.a, libubsan.a)")
    run, tables = standalone["sanitized"]
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.strip() == "%d cases" % len(PINS) and len(tables) == len(PINS)
    for pin, (head, q_off, items, qof, tab) in zip(PINS, tables):
        assert head == pin["shape"] + [pin["backward"], pin["merged"], pin["queues"], pin["count"]], (pin, head)
        assert _digest(items, qof) == pin["sha256"], pin
        if pin["queues"] == 8:
            assert q_off == pin["q_off"], pin


def test_device_table_layout_is_each_queue_in_the_global_start_order(standalone):
    """tk_layout_tables -- what tk_solve uploads -- against the tables test_persistent_solve_queues_drain_whoever_draws_from_them
    derives from queue_of: its "(2) every table holds its items in that order" holds for the device tables too."""
    got = standalone["sanitized"] or _run_standalone(standalone["tmp"], [])
    run, tables = got
    assert run.returncode == 0 and len(tables) == len(PINS), (run.returncode, run.stderr[-4000:])
    for pin, (head, q_off, items, qof, tab) in zip(PINS, tables):
        want_tab, want_off = _queue_major(items, qof, pin["queues"])
        assert q_off == want_off and np.array_equal(tab, want_tab), pin
        assert q_off[8] == pin["count"] and (pin["queues"] == 8 or q_off[1:] == [pin["count"]] * 8)
