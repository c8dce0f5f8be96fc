"""vaporetto_amd/csrc/vocab_count.hpp -- the host side of the vocabulary counter's finish -- as a stand-alone program
(tests/native/vocab_count_test.cpp) built by g++ from that header alone with the address and undefined-behaviour sanitizers and run as a child
process: seeded key sets with tied counts, surfaces of 1- to 4-byte chars, the cuts, output arrays of exactly the stated sizes.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "vocab_count_test.cpp")
CASES = 500


def test_vocab_count_finish_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "vocab_count_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "vaporetto_amd", "csrc"), "-o", exe, SRC])
    r = subprocess.run([exe, str(CASES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    print(r.stdout.decode(), r.stderr.decode())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.decode().split() == ["ok", str(CASES)]
