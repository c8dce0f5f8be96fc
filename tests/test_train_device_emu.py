"""The trainer's device-resident add calls on the CPU emulator (tests/native/hipemu): the checks of tests/traindevsuite.py -- the
device parsers' output straight into the trainer, text anywhere in a larger buffer, the shapes the staged host path never presents,
append order, tagged batches, and the refusals that leave the trainer as it was."""
import ctypes as C
import gc

import pytest

from tests import devmem, emu, kat, traindevsuite, trainsuite
from vaporetto_amd import _lib
from vaporetto_amd.modelfmt import encode_model


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    devmem.EMULATED = True
    yield
    gc.collect()
    devmem.EMULATED = False
    _lib._lib = saved


@pytest.fixture(scope="module")
def ctx(emulated):
    lib = _lib._lib
    raw = encode_model(kat.predictor_test_model())
    pred, batch = C.c_void_p(), C.c_void_p()
    assert lib.vpt_predictor_create(raw, len(raw), 0, 0, C.byref(pred)) == 0
    assert lib.vpt_batch_create(pred, C.byref(batch)) == 0
    yield lib, pred, batch
    lib.vpt_batch_destroy(batch)
    lib.vpt_predictor_destroy(pred)


@pytest.mark.parametrize("case", [trainsuite.CASES[0], trainsuite.CASES[2]])
def test_parser_output_into_trainer_without_a_sync(ctx, case):
    traindevsuite.check_parser_into_trainer(ctx, case)


def test_text_anywhere_in_a_larger_buffer():
    traindevsuite.check_placement(trainsuite.CASES[0])


@pytest.mark.parametrize("name", sorted(traindevsuite.shapes()))
def test_shapes(name):
    traindevsuite.check_shape(name)


def test_batches_without_a_boundary_or_a_sentence():
    traindevsuite.check_no_boundary_batches()


def test_device_and_host_adds_in_alternation():
    traindevsuite.check_append_order(trainsuite.CASES[0])


@pytest.mark.parametrize("kind", ["tokenized", "partial"])
def test_tagged_parser_output_into_trainer(ctx, kind):
    traindevsuite.check_tagged_from_parser(ctx, kind)


def test_tagged_parser_output_into_trainer_l1(ctx):
    traindevsuite.check_tagged_from_parser(ctx, "tokenized", l1=True)


def test_tagged_text_anywhere_in_a_larger_buffer():
    traindevsuite.check_tagged_placement()


@pytest.mark.parametrize("name", traindevsuite.REFUSALS)
def test_refusal_leaves_the_trainer_as_it_was(name):
    traindevsuite.check_refusal(name, tagged=False)


@pytest.mark.parametrize("name", traindevsuite.TAG_REFUSALS)
def test_tagged_refusal_leaves_the_trainer_as_it_was(name):
    traindevsuite.check_refusal(name, tagged=True)
