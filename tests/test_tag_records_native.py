"""vaporetto_amd/csrc/tag_records.h -- the one view of fill_tags' records and the accessors every reader of them goes through: the runs' bound
(a slice of records never leaves the arrays, whatever run_pref holds), the records' count, the one binary search -- held to seeded random
hand-overs by tests/native/tag_records_test.cpp: a stand-alone program built by g++ from that header alone (the vector types come from the
emulator's stand-in for the HIP header), with the address and undefined-behaviour sanitizers, and run as a child process.  Its run_pref and
records arrays are exactly n_runs + 1 and capacity entries long.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tag_records_test.cpp")
CASES = 3000   # five kinds of run_pref in turn, sorted and unsorted records under each; 24 slices a case, 6 searches a slice


def test_accessors_keep_the_bound_and_agree_with_a_linear_scan(tmp_path):
    exe = str(tmp_path / "tag_records_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "vaporetto_amd", "csrc"), "-isystem", os.path.join(ROOT, "tests", "native", "hipemu"), "-o", exe, SRC])
    r = subprocess.run([exe, str(CASES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    print(r.stdout.decode(), r.stderr.decode())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    ok, cases, slices, searches = r.stdout.decode().split()
    assert ok == "ok" and int(cases) == CASES and int(slices) == 24 * CASES and int(searches) == 6 * 24 * CASES
