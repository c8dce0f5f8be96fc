"""The class table the grapheme kernel reads (vaporetto_amd/csrc/tables.cpp: grapheme_table_host), built by g++ on the host and walked over
every scalar value against grapheme_detail::class_of (tests/native/grapheme_table_check.cpp).  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vaporetto_amd", "csrc")


def test_two_stage_table_equals_class_of_on_every_scalar_value(tmp_path):
    exe = str(tmp_path / "grapheme_table_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "grapheme_table_check.cpp"), os.path.join(CSRC, "tables.cpp"), os.path.join(CSRC, "model.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120).stdout.decode()
    print(out)
    lines = out.split("\n")
    assert lines[-2] == "ok", out
    n_bytes = int(lines[0].split()[1])
    assert n_bytes < 64 * 1024   # a few tens of KB: resident in L2
