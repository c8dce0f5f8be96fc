"""The parsers' shared frame on the MI355X: parse_lines_kernel (kernels_parse.hip) through both syntaxes and the C ABI -- the checks of
tests/parsesuite.py."""
import pytest

from tests import kat, parsesuite
from vaporetto_amd import _lib, api
from vaporetto_amd.modelfmt import encode_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    predictor = api.Predictor(api.Model.read_slice(encode_model(kat.predictor_test_model()))[0], False, device=0)
    batch = api.DeviceBatch(predictor)
    yield _lib.load(), predictor._h, batch._h


@pytest.mark.parametrize("kind", parsesuite.KINDS)
def test_window_edges(ctx, kind):
    parsesuite.check_window_edges(ctx, kind)


@pytest.mark.parametrize("kind", parsesuite.KINDS)
def test_grid_stride_loop(ctx, kind):
    parsesuite.check_grid_stride(ctx, kind)


def test_tokenized_first_error_per_reason(ctx):
    parsesuite.check_tokenized_first_errors(ctx)
