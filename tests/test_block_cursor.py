"""BlockCursor of csrc/decim_cursor.h, the squelch stage's stream position on the host: the offset into the block in
progress, the blocks a call completes, the ping-pong half and the fresh flag over cuts of a stream into up to four
calls, against a direct count of the block ends (tests/cpp/block_cursor_test.cpp, which lists the cases).  Host code
only, a stand-alone program built with the undefined-behaviour sanitizer and libstdc++'s bounds assertions: the cursor
is integer arithmetic, and the program's own tables are std::vectors."""
import os
import subprocess

from conftest import ROOT


def test_block_cursor_against_direct_count(tmp_path):
    exe = tmp_path / "block_cursor_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined",
                    "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS",
                    f"-I{os.path.join(ROOT, 'sdr-for-android-lib_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "cpp", "block_cursor_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr
