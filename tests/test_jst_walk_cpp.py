"""The C++ side of the pan-genome index's walk: which symbols a (block, haplotype) cell owns and what its context spells,
libspm_amd/csrc/jst_walk_core.hpp -- the code the build and fan-out kernels call -- through tests/cpp/jst_walk_core_cases: the
header alone, no device, as a stand-alone program, also under AddressSanitizer + UndefinedBehaviorSanitizer, against
haplotypes materialised by brute application of literal allele tables.  The program is compiled here, into the test's own
directory.  Its statistics line is what tests/test_gpu_jst_edges.py asserts of the device index of the same tree."""
import re
import subprocess

import numpy as np
import pytest

import jst_edges as E
from cpp_programs import LIB, build_cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_jst_walk_core_cases(tmp_path, sanitize):
    exe = build_cases("jst_walk_core_cases.cpp", tmp_path, include=[LIB + "/csrc"], sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 50000, r.stdout
    m = re.search(r"stats n_ref 96 H 3 L 16 window 8: (.*)", r.stdout)
    words = m.group(1).split()
    assert dict(zip(words[0::2], map(int, words[1::2]))) == E.WALK_STATS


def test_the_python_table_is_the_programs():
    """the literal of jst_edges.walk_tree is legal, and its haplotypes have the lengths the program's statistics imply"""
    ref, alleles, pool, cov, n_hap = E.walk_tree()
    assert E.legal(len(ref), alleles, cov) and len(ref) == E.WALK_REF and int(ref.max()) < 4
    clamped = np.minimum(alleles["ref_len"].astype(np.int64), len(ref) - alleles["pos"].astype(np.int64))
    total = sum(len(ref) + sum(int(alleles["alt_len"][i]) - int(clamped[i]) for i in range(len(alleles)) if h in E.carriers(cov, i))
                for h in range(n_hap))
    assert total == E.WALK_STATS["haplotype_symbols"]
