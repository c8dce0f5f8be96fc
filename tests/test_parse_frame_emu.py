"""The parsers' shared frame on the CPU emulator (tests/native/hipemu): parse_lines_kernel (kernels_parse.hip) through both syntaxes -- the checks
of tests/parsesuite.py, but for the grid-stride batch: 32 773 lines take the emulator about ten seconds a syntax, so that one runs on the MI355X alone."""
import ctypes as C
import gc

import pytest

from tests import devmem, emu, kat, parsesuite
from vaporetto_amd import _lib
from vaporetto_amd.modelfmt import encode_model


@pytest.fixture(scope="module")
def ctx():
    saved = _lib._lib
    lib = _lib._lib = emu.load()
    devmem.EMULATED = True
    raw = encode_model(kat.predictor_test_model())
    pred, batch = C.c_void_p(), C.c_void_p()
    assert lib.vpt_predictor_create(raw, len(raw), 0, 0, C.byref(pred)) == 0
    assert lib.vpt_batch_create(pred, C.byref(batch)) == 0
    yield lib, pred, batch
    lib.vpt_batch_destroy(batch)
    lib.vpt_predictor_destroy(pred)
    gc.collect()
    devmem.EMULATED = False
    _lib._lib = saved


@pytest.mark.parametrize("kind", parsesuite.KINDS)
def test_window_edges(ctx, kind):
    parsesuite.check_window_edges(ctx, kind)


def test_tokenized_first_error_per_reason(ctx):
    parsesuite.check_tokenized_first_errors(ctx)
