"""Vocabulary ids of the token stream on the CPU emulator (tests/native/hipemu): the vocabulary handle, token_ids_kernel, the one host call and the
tokenizer class against the restatement of tests/vocabref.py -- the checks of tests/vocabsuite.py.  The hostile CSRs run in a child process
(hipemu checks the red zones around every allocation when the workspace goes, and aborts when one is touched)."""
import gc
import os
import subprocess
import sys

import pytest

from tests import devmem, emu, vocabsuite
from vaporetto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    devmem.EMULATED = True
    vocabsuite._PRED.clear()
    yield
    vocabsuite._PRED.clear()
    gc.collect()
    devmem.EMULATED = False
    _lib._lib = saved


@pytest.mark.parametrize("fullwidth", [False, True])
def test_random_documents_match_restatement_unfiltered_and_filtered(fullwidth):
    vocabsuite.check_random(41, fullwidth)


def test_tokens_and_empty_documents_on_both_sides_of_every_tile_edge():
    vocabsuite.check_edges()


def test_length_bound():
    vocabsuite.check_length_bound()


def test_probe_chains_shared_home_slot_and_wrap_around():
    vocabsuite.check_probing()


def test_fingerprint_twin_that_is_no_key_is_unknown():
    vocabsuite.check_verification()


def test_handle_unk_ids_sizes_and_surfaces():
    vocabsuite.check_handle()


def test_errors():
    vocabsuite.check_errors()


def test_one_call_pipeline_equals_the_steps_and_does_not_depend_on_chunks():
    vocabsuite.check_pipeline()


def test_hostile_csr_is_an_error_at_sync_and_touches_nothing_outside():
    r = subprocess.run([sys.executable, "-m", "tests.vocabsuite", "--emu-hostile"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode()
    print(out, r.stderr.decode()[-3000:])
    assert r.returncode == 0, (out[-500:], r.stderr.decode()[-2000:])
    assert out.strip().endswith("ran %d cases" % vocabsuite.N_HOSTILE)
