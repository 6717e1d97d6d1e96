"""csrc/decim_cursor.h's ResampleCursor, the resampler's stream position on the host: first_output, n_out, q0, phi0, the
ping-pong half and the fresh flag over every cut of a stream into up to three calls, against a direct count of the
outputs, near 0 and at 2^62 (tests/cpp/resample_cursor_test.cpp, which lists the cases)."""
import os
import subprocess

from conftest import ROOT


def test_resample_cursor_against_direct_count(tmp_path):
    exe = tmp_path / "resample_cursor_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    f"-I{os.path.join(ROOT, 'sdr-for-android-lib_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "cpp", "resample_cursor_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr
