"""vaporetto_amd/csrc/tag_vocab.hpp -- the host builder of a predictor's tag vocabulary -- as a stand-alone program (tests/native/tag_vocab_test.cpp)
built by g++ from that header alone with the address and undefined-behaviour sanitizers and run as a child process: well-formed tables against a
plain walk, hostile tables without a read outside the arrays.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tag_vocab_test.cpp")
CASES = 3000


def test_vocabulary_builder_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "tag_vocab_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "vaporetto_amd", "csrc"), "-o", exe, SRC])
    r = subprocess.run([exe, str(CASES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    print(r.stdout.decode(), r.stderr.decode())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.decode().split() == ["ok", str(CASES)]
