"""CPU suite: the registry of the timing entries (tests/timing_entries.py) against the header, the GPU test file and c_api.cpp -- no GPU, no library."""
import os
import re

import timing_entries as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(rel):
    with open(os.path.join(ROOT, rel)) as f:
        return f.read()


def _gpu_tests():
    """test name -> source text of the test function (up to the next top-level statement)"""
    src = _read(reg.GPU_FILE)
    heads = [(mt.group(1), mt.start()) for mt in re.finditer(r"^def (test_\w+)\(", src, re.M)]
    ends = [mt.start() for mt in re.finditer(r"^(?:def |@|class |[A-Za-z_])", src, re.M)]
    out = {}
    for name, at in heads:
        later = [e for e in ends if e > at]
        out[name] = src[at:later[0] if later else len(src)]
    return out


def _check_entries():
    header = _read(reg.HEADER)
    declared = re.findall(reg.PROTOTYPE, header, re.M)
    assert len(declared) >= 7 and len(set(declared)) == len(declared), declared
    missing = [name for name in declared if name not in reg.TIMING_ENTRIES]
    assert not missing, f"timing entries of {reg.HEADER} without a row in tests/timing_entries.py: {missing}"
    gone = [name for name in reg.TIMING_ENTRIES if name not in declared]
    assert not gone, f"tests/timing_entries.py names prototypes {reg.HEADER} does not declare: {gone}"
    tests = _gpu_tests()
    gpu_src = _read(reg.GPU_FILE)
    assert re.search(r"^pytestmark = pytest\.mark\.gpu$", gpu_src, re.M)
    for name, named in reg.TIMING_ENTRIES.items():
        assert named, f"{name}: no test registered"
        for t in named:
            assert t in tests, f"{name}: {t} is not a test of {reg.GPU_FILE}"
        # the GPU file reaches the C entries through one table (ENTRY_SYMBOLS): the entry must be in it
        assert re.search(r'"%s"' % re.escape(name), gpu_src), f"{reg.GPU_FILE} never names {name}"


def _check_reset_forms():
    src = _read(reg.SOURCE)
    tests = _gpu_tests()
    for what, pattern, named, _ in reg.RESET_FORMS:
        assert re.search(pattern, src), f"{what}: the condition is no longer in {reg.SOURCE} as registered -- re-register what crosses it"
        assert named, what
        for t in named:
            assert t in tests, f"{what}: {t} is not a test of {reg.GPU_FILE}"
    # both readers of SPMV_ACC_RESET_NT (the per-launch body and the kernel-clock entry) are still there
    assert len(re.findall(r'std::getenv\("SPMV_ACC_RESET_NT"\)', src)) == 2
    assert len(re.findall(r'std::getenv\("SPMV_ACC_RESET_MEMCPY"\)', src)) == 1


def test_every_timing_entry_and_reset_form_is_registered():
    _check_entries()
    _check_reset_forms()
