"""The factor store's host side (gpmp_amd/csrc/factor_store.h) without a GPU: tests/factor_store_host.cpp drives the key
comparison, the budget arithmetic and one entry through publish / hit / miss / invalidate / release with the device calls stubbed
out.  It is a stand-alone program built with AddressSanitizer + UBSan on the host and run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_factor_store_bookkeeping_under_the_host_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    exe = str(tmp_path / "factor_store_host")
    src = os.path.join(ROOT, "tests", "factor_store_host.cpp")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FACTOR-STORE-HOST-OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]


def test_switch_is_documented_and_adds_no_symbol():
    """GPMP_FACTOR_STORE_MB is in the switch table of DESIGN.md; the store is reached through existing entry points only."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "`GPMP_FACTOR_STORE_MB`" in design
    header = open(os.path.join(ROOT, "include", "gpmp_hip.h")).read()
    assert "factor_store" not in header
