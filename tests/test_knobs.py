"""CPU: the environment knobs the library reads are exactly the ones DESIGN.md section 7 lists, and every SPM_HIP_* name
that the tests and scripts use is one the library reads (a misspelt or retired name would silently test nothing)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_KNOBS = {"SPM_HIP_CHECK", "SPM_HIP_H"}  # an error-check macro and the C header's include guard


def _tokens(pattern, *globs):
    files = [f for g in globs for f in glob.glob(os.path.join(ROOT, g), recursive=True) if os.path.isfile(f)]
    return {t for f in files for t in re.findall(pattern, open(f, encoding="utf-8").read())} - NOT_KNOBS


def _read_by_library():
    return _tokens(r'(?:env_int|getenv)\(\s*"(SPM_HIP_[A-Z0-9_]+)"', "libspm_amd/csrc/*.hip", "libspm_amd/csrc/*.hpp",
                   "libspm_amd/csrc/*.cpp", "include/**/*.h", "include/**/*.hpp")


def test_library_reads_exactly_the_documented_knobs():
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    rows = [line for line in design[design.index("## 7. "):design.index("## 8. ")].splitlines() if line.startswith("| `")]
    assert _read_by_library() == {t for line in rows for t in re.findall(r"SPM_HIP_[A-Z0-9_]+", line)}


def test_tests_and_scripts_only_name_knobs_the_library_reads():
    used = _tokens(r"SPM_HIP_[A-Z0-9_]+", "tests/**/*.py", "tests/**/*.cpp", "scripts/*")
    assert used <= _read_by_library(), sorted(used - _read_by_library())
