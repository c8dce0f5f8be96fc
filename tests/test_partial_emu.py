"""Partial annotation on the CPU emulator (tests/native/hipemu): parse_lines_kernel<PartialSyntax> / write_partial_kernel (kernels_parse.hip) and their host
pipelines against the restatement -- the checks of tests/partialsuite.py."""
import ctypes as C
import gc

import pytest

from tests import devmem, emu, kat, partialsuite
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


def test_parity_host_and_device_every_array(ctx):
    partialsuite.check_parity(ctx, 120)


def test_quirks(ctx):
    partialsuite.check_quirks(ctx)


def test_no_line_and_one_line(ctx):
    partialsuite.check_small_batches(ctx)


def test_capacity_exact_and_one_short(ctx):
    partialsuite.check_capacity(ctx)


def test_errors_first_error_of_the_smallest_line(ctx):
    partialsuite.check_errors(ctx, 40)


def test_mutated_batch(ctx):
    partialsuite.check_mutated(ctx, 120)


def test_writer_hand_built_csr(ctx):
    partialsuite.check_writer(ctx)


def test_determinism_and_reuse(ctx):
    partialsuite.check_determinism_and_reuse(ctx)
