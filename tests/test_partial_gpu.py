"""Partial annotation on the MI355X: parse_lines_kernel<PartialSyntax> / write_partial_kernel (kernels_parse.hip) through the C ABI and through
api.Predictor -- the checks of tests/partialsuite.py."""
import numpy as np
import pytest

from tests import kat, partialsuite
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


def test_parity_host_and_device_every_array(ctx):
    partialsuite.check_parity(ctx, 400)


def test_quirks(ctx):
    partialsuite.check_quirks(ctx)


def test_no_line_and_one_line(ctx):
    partialsuite.check_small_batches(ctx)


def test_capacity_exact_and_one_short(ctx):
    partialsuite.check_capacity(ctx)


def test_errors_first_error_of_the_smallest_line(ctx):
    partialsuite.check_errors(ctx, 40)


def test_mutated_batch(ctx):
    partialsuite.check_mutated(ctx, 400)


def test_writer_hand_built_csr(ctx):
    partialsuite.check_writer(ctx)


def test_determinism_and_reuse(ctx):
    partialsuite.check_determinism_and_reuse(ctx)


def test_predictor_methods(predictor):
    """api.Predictor.parse_partial_packed / write_partial_packed return what the host forms return"""
    structs, lines = partialsuite.parity_batch(120)
    lines = lines[:40]
    utf8, boff = partialsuite.pack(lines)
    p = predictor.parse_partial_packed(utf8, boff)
    h = api.parse_partial_host([ln.encode("utf-8") for ln in lines])
    partialsuite.assert_same(p, h, "packed")
    a = [p[k] for k in ("raw", "raw_offsets", "out_offsets", "labels", "n_tags", "tag_index", "span_offsets", "tag_bytes")]
    text, toff = predictor.write_partial_packed(*a)
    htext, htoff = api.write_partial_host(*a)
    assert bytes(text) == bytes(htext) and np.array_equal(toff, htoff)
    assert bytes(predictor.write_partial_packed(*a[:4])[0]) == bytes(api.write_partial_host(*a[:4])[0])
    with pytest.raises(api.VaporettoError) as e:
        predictor.parse_partial_packed(*partialsuite.pack(["a|b", "a\\漢"]))
    assert str(e.value) == "InvalidArgumentError: partial_annotation_text: contains an invalid boundary character: '漢' (line 1)"
