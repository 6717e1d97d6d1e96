"""csrc/decim_cursor.h, the stream position the DDC, the demodulator and the channelizer share on the host: first,
n_out, the ping-pong half and the fresh flag over cuts of a stream into up to four calls, against a direct count of
the multiples of D (tests/cpp/decim_cursor_test.cpp, which lists the cases)."""
import os
import subprocess

from conftest import ROOT


def test_decim_cursor_against_direct_count(tmp_path):
    exe = tmp_path / "decim_cursor_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    f"-I{os.path.join(ROOT, 'sdr-for-android-lib_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "cpp", "decim_cursor_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr
