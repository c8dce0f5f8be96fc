"""The token-stream feature on the CPU emulator (tests/native/hipemu): the span kernel, the linebreaks-first label step and the host pipeline
of vpt_token_stream_batch against the restatement of tests/tokenref.py -- the checks of tests/tokensuite.py."""
import gc

import pytest

from tests import devmem, emu, tokensuite
from vaporetto_amd import _lib


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    devmem.EMULATED = True
    yield
    gc.collect()
    devmem.EMULATED = False
    _lib._lib = saved


NO_G = [c for c in tokensuite.KAT["cases"] if "G" not in c["wsconst"]]


@pytest.mark.parametrize("case", NO_G, ids=[c["name"] for c in NO_G])
def test_adapter_kats_through_the_c_abi(case):
    tokensuite.check_kat_cabi(case)


@pytest.mark.parametrize("case", tokensuite.KAT["cases"], ids=[c["name"] for c in tokensuite.KAT["cases"]])
def test_adapter_kats_through_the_tokenizer(case):
    tokensuite.check_kat_tokenizer(case)


@pytest.mark.parametrize("wc,wt", tokensuite.WINDOWS)
def test_random_models_and_documents_match_restatement(wc, wt):
    tokensuite.check_random(11 + wc, wc, wt)


def test_spans_of_caller_labels():
    tokensuite.check_caller_labels(3)


def test_spans_equal_what_tokenize_batch_implies():
    tokensuite.check_consistency_with_tokenize(9)


def test_errors():
    tokensuite.check_errors()
