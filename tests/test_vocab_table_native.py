"""vaporetto_amd/csrc/vocab_table.hpp -- the host builder of the id pass's vocabulary -- as a stand-alone program (tests/native/vocab_table_test.cpp)
built by g++ from that header (and pattern_tagger.hpp's hash) with the address and undefined-behaviour sanitizers and run as a child process:
seeded vocabularies, the load-factor bounds, every key found and every non-key not, the rejections by message.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "vocab_table_test.cpp")
CASES = 2000


def test_vocab_table_builder_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "vocab_table_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "vaporetto_amd", "csrc"), "-o", exe, SRC])
    r = subprocess.run([exe, str(CASES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    print(r.stdout.decode(), r.stderr.decode())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.decode().split() == ["ok", str(CASES)]
