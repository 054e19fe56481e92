"""The seed index build (libspm_amd/csrc/index_build.hpp and the headers it gathers) without a device, pinned bit for bit:
tests/cpp/index_build_cases builds some thirty needle sets with 1 and with 4 threads and prints, per build, the plan and a
digest over every field and vector of the resulting seed_index; tests/golden/index_build/digests.txt holds what the commit
named there printed, and every line is compared with its own recorded line.  tests/cpp/index_plan_cases checks the
planner's pure decisions on rows worked out by hand.  Both also under AddressSanitizer + UndefinedBehaviorSanitizer (stand-
alone programs, run directly).  The programs are compiled here, into the test's own directory."""
import os
import re
import subprocess

import pytest

from cpp_programs import LIB, ROOT, build_cases

GOLDEN = os.path.join(ROOT, "tests", "golden", "index_build", "digests.txt")
SANITIZE = pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])


def _run(source, out_dir, sanitize):
    exe = build_cases(source, out_dir, std="c++17", include=[os.path.join(LIB, "csrc")], sanitize=sanitize, threads=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    return r.stdout


def _plans(lines):
    """case -> the plan fields of its 1-thread line"""
    plans = {}
    for line in lines:
        name, *fields = line.split()
        f = dict(x.split("=") for x in fields)
        if f["threads"] == "1":
            plans[name] = {k: int(v) for k, v in f.items() if k != "digest"}
    return plans


@SANITIZE
def test_index_build_matches_the_recorded_digests(tmp_path, sanitize):
    with open(GOLDEN) as f:
        golden = [x for x in f.read().splitlines() if x and not x.startswith("#")]
    lines = _run("index_build_cases.cpp", tmp_path, sanitize).splitlines()
    assert len(lines) == len(golden) and len(lines) >= 2 * 30
    for got, want in zip(lines, golden):
        assert got == want
    # between them the cases reach every branch of the planner: read off what was printed, not assumed
    P = _plans(lines)

    def plan(name, **want):
        return all(P[name][k] == v for k, v in want.items())

    assert all(p["rc"] == 0 for p in P.values())
    assert plan("c3_shape", passes=1, stride=8, key_len=16, anchored=0, dense=0, variant=2)      # one pass, fingerprint table
    assert plan("stride2_short_seeds", passes=1, stride=2, key_len=14, variant=4)               # presence bits
    assert plan("k64_band_merging", passes=1, stride=2, dense=0)
    assert plan("no_filter", passes=0)                                                          # seeds shorter than any key
    assert plan("sub_batches", passes=5, stride=2, anchored=0, dense=0)                         # the cost model, sub-batches
    assert plan("anchored", passes=3, stride=1, anchored=1, variant=2)
    assert plan("anchored_table_fails", passes=4, stride=1, anchored=1, variant=1)              # all three attempts spent
    assert plan("overfull_table", passes=1, stride=4, variant=2)                                # re-partitioned (stride 8 first)
    assert plan("bloom_cascade", passes=1, variant=1)
    assert plan("dense_by_default", passes=1, stride=1, dense=1, variant=3)
    assert plan("dense_forced_64", dense=1, variant=3) and plan("dense_forced_100", dense=1, variant=3)
    assert plan("shiftor_32", passes=1, stride=16)
    assert plan("whole_seed_keys", passes=1, stride=1, key_len=11)
    assert plan("too_dense_short_keys", passes=0)                                               # kMaxSurvivorShare
    assert plan("dna5_with_n", passes=1, variant=2) and plan("dna15", passes=1, variant=2)
    assert plan("dna5_needle_without_seeds", passes=0)                                          # a needle without a layout
    assert plan("dna5_bloom_cascade", passes=0) and plan("dna5_table_fails", passes=0)          # a pass that is not ok
    assert plan("repeats_sparse", passes=1, dense=0) and plan("repeats_dense", dense=1)
    assert plan("dense_declined", passes=3, dense=0)                                            # dense wanted, not possible
    assert plan("unanchored_stride1", passes=3, stride=1, anchored=0, dense=0)
    assert plan("too_many_passes", passes=0)                                                    # kMaxPasses
    assert plan("needle_too_long", passes=0)
    assert {p["variant"] for p in P.values()} == {0, 1, 2, 3, 4}
    assert {p["stride"] for p in P.values()} == {0, 1, 2, 4, 8, 16}


@SANITIZE
def test_index_plan_cases(tmp_path, sanitize):
    out = _run("index_plan_cases.cpp", tmp_path, sanitize)
    m = re.search(r"(\d+) checks, 0 failures", out)
    assert m and int(m.group(1)) >= 40, out
