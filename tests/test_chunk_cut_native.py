"""vaporetto_amd/csrc/host_chunks.hpp -- how the host-buffer pipelines cut a batch into chunks, and the sizes they take from the cuts (the
chunks at most, the pinned words staged, the slots of the device offsets) -- held to seeded random batches by tests/native/chunk_cut_test.cpp:
a stand-alone program built by g++ from that header alone, with the address and undefined-behaviour sanitizers, and run as a child process.
Its staging arrays are exactly as long as the header's bounds say.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "chunk_cut_test.cpp")
BATCHES = 4000   # x 3 cutters; chunk sizes 1, 7, 50 and larger than the batch in turn, five kinds of batch under each


def test_cutters_partition_and_keep_their_bounds(tmp_path):
    exe = str(tmp_path / "chunk_cut_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "vaporetto_amd", "csrc"), "-o", exe, SRC])
    r = subprocess.run([exe, str(BATCHES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    print(r.stdout.decode(), r.stderr.decode())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    ok, batches, cuts, chunks = r.stdout.decode().split()
    assert ok == "ok" and int(batches) == BATCHES and int(cuts) == 3 * BATCHES
    assert int(chunks) > 10 * BATCHES   # the small chunk sizes cut: many chunks per batch on average
