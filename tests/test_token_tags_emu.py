"""Tags in the token stream on the CPU emulator (tests/native/hipemu): the tag vocabulary, token_spans_kernel<true>, the stop filter's kernels and
handle, vpt_token_stream_tagged_batch and the tokenizer class against the restatement of tests/tokentagref.py -- the checks of
tests/tokentagsuite.py.  The hostile offsets run in child processes (hipemu checks the red zones around every allocation when the workspace
goes, and aborts when one is touched)."""
import gc
import os
import subprocess
import sys

import pytest

from tests import devmem, emu, tagoffsetsuite, tokentagsuite
from vaporetto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    devmem.EMULATED = True
    yield
    gc.collect()
    devmem.EMULATED = False
    _lib._lib = saved


def test_vocabulary_is_the_walk_of_the_model_and_survives_save_load():
    tokentagsuite.check_vocabulary()


@pytest.mark.parametrize("n_tags", [1, 3])
def test_random_documents_match_restatement(n_tags):
    tokentagsuite.check_random(21 + n_tags, n_tags)


def test_tagged_tokens_on_both_sides_of_every_edge():
    tokentagsuite.check_edges()


def test_no_record_every_record_and_no_tag_models():
    tokentagsuite.check_no_record_and_every_record()


def test_errors():
    tokentagsuite.check_errors()


@pytest.mark.parametrize("variant", ["plain", "pattern"])
@pytest.mark.parametrize("batch", tagoffsetsuite.BATCHES)
def test_hostile_out_offsets_are_an_error_at_sync_and_write_nothing_outside(batch, variant):
    r = subprocess.run([sys.executable, "-m", "tests.tokentagsuite", "--emu-hostile", batch, variant], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode()
    print(out, r.stderr.decode()[-3000:])
    assert r.returncode == 0, (out[-500:], r.stderr.decode()[-2000:])
    assert out.strip().endswith("ran %d cases" % tagoffsetsuite.CASES_PER_BATCH[batch])


def test_stream_and_stop_filter_match_restatement():
    tokentagsuite.check_stream()


def test_tokenizer_class_and_deserialize():
    tokentagsuite.check_tokenizer()


def test_stop_and_stream_errors():
    tokentagsuite.check_stop_errors()


def test_filter_keeps_and_drops_on_both_sides_of_every_edge():
    tokentagsuite.check_filter_edges()


def test_filter_entry_with_hostile_offsets_and_capacities_writes_nothing_outside():
    r = subprocess.run([sys.executable, "-m", "tests.tokentagsuite", "--emu-filter"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode()
    print(out, r.stderr.decode()[-3000:])
    assert r.returncode == 0, (out[-500:], r.stderr.decode()[-2000:])
    assert out.strip().endswith("ran 35 cases")
