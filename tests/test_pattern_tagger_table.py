"""PatternMatchTagger's host table builder (vaporetto_amd/csrc/pattern_tagger.cpp) as a stand-alone g++ program: tests/native/rule_table_check.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rule_table_builder(tmp_path):
    exe = str(tmp_path / "rule_table_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "native", "rule_table_check.cpp"),
                           os.path.join(ROOT, "vaporetto_amd", "csrc", "pattern_tagger.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "rule table ok" in out.stdout, out.stdout + out.stderr
