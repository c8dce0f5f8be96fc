"""vaporetto_amd/csrc/scratch_carve.hpp -- the carver that hands out the 256-byte sections of one allocation, the sort-and-scan tail, the radix
pass lists and the five layouts the postings drivers carve out of a workspace's scratch -- held by tests/native/scratch_carve_test.cpp to offsets
and totals written out as data (the hand-written offset chains the drivers had before the carver): a stand-alone program built by g++ from
that header alone, with the address and undefined-behaviour sanitizers, and run as a child process.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "scratch_carve_test.cpp")
# the carver, the pass lists, 8 tails; 4 postings, 32 + 32 merge (plain and positional, ordered and general), 32 search (OR and boolean),
# 8 phrase layouts
LAYOUTS = 2 + 8 + 4 + 64 + 32 + 8


def test_layouts_are_the_bytes_of_the_hand_written_chains(tmp_path):
    exe = str(tmp_path / "scratch_carve_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "vaporetto_amd", "csrc"), "-o", exe, SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    print(r.stdout.decode(), r.stderr.decode())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    ok, layouts, sections = r.stdout.decode().split()
    assert ok == "ok" and int(layouts) == LAYOUTS
    assert int(sections) == 4 * 8 + 16 * (3 + 5) + 16 * (9 + 13) + 32 * 15 + 8 * 17   # the sections a driver had in each case
