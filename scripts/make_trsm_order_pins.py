#!/usr/bin/env python3
"""Pins of the persistent solves' ticket tables -> tests/golden/trsm_order_pins.json (no GPU, seconds).

Run it on a build of the commit whose tables are to be held (the file records that commit's id): it goes through the C ABI only
(nngp_trsm_ticket_queues), so it says what that library schedules, not what some copy of the scheduler would.  Per case: the item
count, the sha256 of the little-endian int32 stream [word, r, c, J] per item followed by queue_of, and for eight queues q_off[0..8]
of the queue-major device table (queue q = the items with queue_of == q, in the global start order).
tests/test_trsm_order_host.py holds the library and a sanitized stand-alone build of csrc/trsm_order.cpp to these.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "trsm_order_pins.json")

# (row tiles, block columns, tail tiles, workers): the shapes of test_persistent_solve_ticket_tables_only_wait_on_lower_tickets, of
# test_persistent_solve_queues_drain_whoever_draws_from_them (256 workers), and four more (deep, wide, smallest pair, odd everything)
SHAPES = [(8, 32, 8, 512), (1, 2, 8, 512), (2, 3, 1, 16), (29, 11, 5, 512), (8, 8, 8, 512), (3, 10, 8, 1), (8, 64, 8, 512), (5, 9, 3, 97),
          (8, 32, 8, 256), (8, 8, 8, 256), (4, 16, 8, 256), (29, 11, 5, 256), (16, 6, 8, 256), (3, 5, 2, 256), (1, 3, 8, 256),
          (8, 32, 8, 256), (64, 2, 1, 256), (2, 2, 8, 256), (3, 4, 7, 256)]


def table(lib, mt, nb, tail, backward, workers, merged, queues):
    count = ctypes.c_int64(0)
    assert lib.nngp_trsm_ticket_queues(mt, nb, tail, backward, workers, merged, queues, None, None, 0, ctypes.byref(count)) == 0, lib.nngp_last_error()
    items = np.zeros((count.value, 4), np.int32)
    qof = np.zeros(count.value, np.int32)
    assert lib.nngp_trsm_ticket_queues(mt, nb, tail, backward, workers, merged, queues, items.ctypes.data_as(ctypes.c_void_p),
                                       qof.ctypes.data_as(ctypes.c_void_p), count.value, ctypes.byref(count)) == 0, lib.nngp_last_error()
    return items, qof


def digest(items, qof):
    return hashlib.sha256(np.ascontiguousarray(items, "<i4").tobytes() + np.ascontiguousarray(qof, "<i4").tobytes()).hexdigest()


def q_offsets(qof):
    return [0] + np.cumsum(np.bincount(qof, minlength=8)).tolist()


def main():
    from nngp_src_amd import _lib
    lib = _lib.load()
    commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "nngp-src_amd/csrc"], text=True).strip()
    assert not dirty, "the library's sources differ from the commit that would be recorded:\n" + dirty
    cases = []
    for mt, nb, tail, workers in dict.fromkeys(SHAPES):
        for backward in (0, 1):
            for merged in (1, 0):
                for queues in (1, 8):
                    items, qof = table(lib, mt, nb, tail, backward, workers, merged, queues)
                    case = {"shape": [mt, nb, tail, workers], "backward": backward, "merged": merged, "queues": queues,
                            "count": int(len(items)), "sha256": digest(items, qof)}
                    if queues == 8:
                        case["q_off"] = q_offsets(qof)
                    cases.append(case)
    with open(OUT, "w") as f:
        f.write('{"generator": "scripts/make_trsm_order_pins.py", "commit": "%s",\n "cases": [\n' % commit)
        f.write(",\n".join("  " + json.dumps(c) for c in cases))
        f.write("\n ]}\n")
    print("wrote %s: %d cases of commit %s" % (OUT, len(cases), commit))


if __name__ == "__main__":
    sys.exit(main())
