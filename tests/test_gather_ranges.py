"""GatherRanges of csrc/gather_ranges.h, the byte ranges that gathers still read and the engine's calls wait for before
they write: the latest gather over any byte of a range, the same range gathered again, and a write that retires a range
only when it covers it whole, against a byte map of a 256-byte arena over every pair of ranges on a 16-byte grid
(tests/cpp/gather_ranges_test.cpp, which lists the cases).  Host code only, a stand-alone program built with the
undefined-behaviour sanitizer and libstdc++'s bounds assertions: the ranges are pointer arithmetic, and both sides keep
their entries in std::vectors."""
import os
import subprocess

from conftest import ROOT


def test_gather_ranges_against_byte_map(tmp_path):
    exe = tmp_path / "gather_ranges_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined",
                    "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS",
                    f"-I{os.path.join(ROOT, 'sdr-for-android-lib_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "cpp", "gather_ranges_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr
