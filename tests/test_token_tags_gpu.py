"""Tags in the token stream on the MI355X through the C ABI: the tag vocabulary, token_spans_kernel<true>, the stop filter, the one host call and
the tokenizer class against the restatement of tests/tokentagref.py -- the checks of tests/tokentagsuite.py.  (The hostile offsets run here
after they have run on the emulator, tests/test_token_tags_emu.py: an error at sync or none, the guard words around every caller array intact.)"""
import pytest

from tests import tagoffsetsuite, tokentagsuite

pytestmark = pytest.mark.gpu


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
    assert tokentagsuite.run_hostile_group(batch, variant) == tagoffsetsuite.CASES_PER_BATCH[batch]


def test_stream_and_stop_filter_match_restatement():
    tokentagsuite.check_stream()


def test_tokenizer_class_and_deserialize():
    tokentagsuite.check_tokenizer()


def test_stop_and_stream_errors():
    tokentagsuite.check_stop_errors()


def test_filter_keeps_and_drops_on_both_sides_of_every_edge():
    tokentagsuite.check_filter_edges()


def test_filter_entry_with_hostile_offsets_and_capacities_writes_nothing_outside():
    assert tokentagsuite.run_filter_hostile() == 35
