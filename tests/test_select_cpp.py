"""The C++ side of hit selection: the host-side plan (libspm_amd/csrc/select_plan.hpp) through tests/cpp/select_plan_cases
(plain asserts, no device), and the mirror's hit_selection overloads through tests/cpp/select_cases -- compiled with the
reference's warning flags, run on the GPU, every printed callback compared with Hits.select() / align() in Python on the
same generated input."""
import os
import re
import subprocess

import numpy as np
import pytest

from cpp_programs import build_cases, build_mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _sources(dirs):
    out = []
    for d in dirs:
        for base, _, files in os.walk(d):
            out += [os.path.join(base, f) for f in files if f.endswith((".hpp", ".h", ".so"))]
    return out


def _build(name, deps, link):
    """g++ the program next to its source unless it is newer than everything it is made of"""
    src, exe = os.path.join(CPP, name + ".cpp"), os.path.join(CPP, name)
    newest = max(os.path.getmtime(f) for f in [src] + deps)
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        if link:
            build_mirror(name + ".cpp", CPP, fixtures=False)
        else:
            build_cases(name + ".cpp", CPP, include=[os.path.join(ROOT, "include")])
    return exe


def _plan_exe():
    return _build("select_plan_cases", [os.path.join(ROOT, "libspm_amd", "csrc", "select_plan.hpp"),
                                        os.path.join(ROOT, "include", "spm_hip.h")], False)


def _mirror_exe():
    return _build("select_cases", _sources([os.path.join(ROOT, "include")]) + [os.path.join(ROOT, "libspm_amd", "libspm_hip.so")], True)


def test_select_plan_cases():
    r = subprocess.run([_plan_exe()], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 1000, r.stdout


def test_mirror_selection_overloads_compile_with_reference_warning_flags():
    assert os.path.exists(_mirror_exe())


M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def mix64(z):
    z = (np.asarray(z, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)) & M64
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M64
    return z ^ (z >> np.uint64(31))


@pytest.mark.gpu
def test_mirror_selected_callbacks_equal_python(spm, ctx):
    r = subprocess.run([_mirror_exe()], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    assert re.search(r"(\d+) checks, 0 failures", r.stdout)

    # the same input here
    N, NEEDLES, L, SEED = 1 << 16, 24, 60, 0x5E1EC7
    with np.errstate(over="ignore"):
        T = (mix64(np.uint64(SEED) + np.arange(N, dtype=np.uint64)) & np.uint64(3)).astype(np.uint8)
        needles, ks = [], []
        for p in range(NEEDLES):
            at = int(mix64(np.uint64(SEED ^ ((p + 1) << 32)))) % (N - L)
            nd = T[at:at + L].copy()
            if p % 2:
                nd[L // 2] = (int(nd[L // 2]) + 1) & 3
            needles.append(nd)
            ks.append(p % 4)
    text = ctx.upload(T)
    ps = ctx.patterns(spm.ALGO_MYERS, needles, k=np.array(ks, dtype=np.uint16))
    h = spm.scan(ctx, text, ps)
    for mode, kw in enumerate((dict(), dict(best=0), dict(window=1, best=1))):
        sel = h.select(**kw)
        v = sel.view()
        al = sel.align()
        ar, ao = al.view(), al.ops
        want_op = [f"op{mode} {int(x['pattern'])} {max(0, int(x['pos']) - L)} {int(x['pos'])} {int(x['score'])}" for x in v]
        want_loc = [f"loc{mode} {int(a['pattern'])} {int(a['begin'])} {int(a['end'])} {int(a['score'])} {al.cigar(i, ar, ao)}"
                    for i, a in enumerate(ar)]
        got_op = [ln for ln in r.stdout.splitlines() if ln.startswith(f"op{mode} ")]
        got_loc = [ln for ln in r.stdout.splitlines() if ln.startswith(f"loc{mode} ")]
        assert len(want_op) > NEEDLES // 2 and got_op == want_op
        assert got_loc == want_loc
    one = ctx.patterns(spm.ALGO_MYERS, [needles[3]], k=3)
    v = spm.scan(ctx, text, one).select().view()
    want = [f"single 3 {max(0, int(x['pos']) - L)} {int(x['pos'])} {int(x['score'])}" for x in v]
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("single ")] == want and want
