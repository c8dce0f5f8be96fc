"""Hostile out_offsets over several front-end runs (tests/tagoffsetsuite.py) on the CPU emulator (tests/native/hipemu).  The cases of a (batch,
variant) run in a child process of their own: hipemu aborts when a red zone around one of its allocations was written, which is what an overrun
of the workspace's own buffers looks like -- here that is a failed test, not a dead pytest."""
import os
import subprocess
import sys

import pytest

from tests import emu, tagoffsetsuite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ran = {}


@pytest.fixture(scope="module", autouse=True)
def emulated_library():
    emu.build_emulated()   # once, here: the children only load it


@pytest.mark.parametrize("variant", tagoffsetsuite.VARIANTS)
@pytest.mark.parametrize("batch", tagoffsetsuite.BATCHES)
def test_hostile_offsets_stay_inside_the_batch(batch, variant):
    r = subprocess.run([sys.executable, "-m", "tests.tagoffsetsuite", "--emu", batch, variant], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    tail = "\n".join(r.stdout.splitlines()[-25:])
    assert r.returncode == 0, "exit status %d (negative: a signal -- 6 is hipemu's abort)\n%s" % (r.returncode, tail)
    started = [ln for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert len(started) == tagoffsetsuite.CASES_PER_BATCH[batch] and ("ran %d cases" % len(started)) in r.stdout, tail
    _ran[(batch, variant)] = len(started)


@pytest.mark.parametrize("batch,variant", [("A", "plain"), ("B", "pattern"), ("C", "scores")])
def test_the_clamps_alone_hold(batch, variant):
    """A build whose front end and pattern tagger do not look at the batch's control word (-DVPT_TAG_NO_OFFSETS_GATE): overlapping runs are accepted,
    counted and scanned, and what keeps every write inside the arrays is the scan's capacity and the consumers' clamps alone."""
    env = dict(os.environ, VPT_EMU_DEFINES="-DVPT_TAG_NO_OFFSETS_GATE")
    r = subprocess.run([sys.executable, "-m", "tests.tagoffsetsuite", "--emu", batch, variant], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-25:])
    assert r.returncode == 0, "exit status %d (negative: a signal -- 6 is hipemu's abort)\n%s" % (r.returncode, tail)
    assert ("ran %d cases" % tagoffsetsuite.CASES_PER_BATCH[batch]) in r.stdout, tail


def test_every_case_ran():
    if len(_ran) != len(tagoffsetsuite.BATCHES) * len(tagoffsetsuite.VARIANTS):
        pytest.skip("a selection of the cases was run")
    assert sum(_ran.values()) == tagoffsetsuite.N_CASES == 123
