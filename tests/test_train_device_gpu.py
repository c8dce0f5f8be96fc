"""The trainer's device-resident add calls on the MI355X: the checks of tests/traindevsuite.py, on torch's current stream and, for the
parser-into-trainer path, on a stream of the caller's own."""
import pytest

from tests import kat, traindevsuite, trainsuite
from vaporetto_amd import _lib, api
from vaporetto_amd.modelfmt import encode_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def predictor():
    return api.Predictor(api.Model.read_slice(encode_model(kat.predictor_test_model()))[0], False, device=0)


@pytest.fixture(scope="module")
def ctx(predictor):
    batch = api.DeviceBatch(predictor)
    yield _lib.load(), predictor._h, batch._h


@pytest.mark.parametrize("case", [trainsuite.CASES[0], trainsuite.CASES[2]])
def test_parser_output_into_trainer_without_a_sync(ctx, case):
    traindevsuite.check_parser_into_trainer(ctx, case)


def test_parser_output_into_trainer_on_the_callers_stream(ctx):
    import torch
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    traindevsuite.check_parser_into_trainer(ctx, trainsuite.CASES[0], s.cuda_stream)
    s.synchronize()


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
