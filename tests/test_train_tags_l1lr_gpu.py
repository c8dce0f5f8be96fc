"""Solver 6 for tag models (Trainer(l1r_lr=True, train_tags=True, l1r_lr_tags=True)) on the MI355X against the
restatement of tests/tagl1lrref.py: the in-kernel solver of vaporetto_amd/csrc/kernels_train_tags_l1lr.hip and the group launches of
solve_l1r_lr over a tag problem's own matrix, the stats, the model's bytes, determinism, the shapes at which the kernel takes another
path, the round trip through the predictor against the CPU oracle, and the errors."""
import pytest

from tests import tagl1lrsuite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def own_trainers():
    tagl1lrsuite.trained.cache_clear()   # a trainer belongs to the library that made it
    yield
    tagl1lrsuite.trained.cache_clear()


CASES = [(name, path) for name in sorted(tagl1lrsuite.CASES) for path in (0, 1)]


@pytest.mark.parametrize("name,path", CASES)
def test_objective_violation_counts_and_mirror(name, path):
    stats = tagl1lrsuite.check_solution(name, path)
    assert {p["path"] for p in stats["problems"]} == ({1} if path == 0 else {2})


@pytest.mark.parametrize("name,path", CASES)
def test_library_stats(name, path):
    tagl1lrsuite.check_library_stats(name, path)


@pytest.mark.parametrize("name", sorted(tagl1lrsuite.CASES))
def test_paths_agree(name):
    tagl1lrsuite.check_paths_agree(name)


@pytest.mark.parametrize("name,path", CASES)
def test_model_bytes_determinism_and_sparsity(name, path):
    tagl1lrsuite.check_model(name, path)


def test_other_solvers_unchanged_by_the_flag():
    tagl1lrsuite.check_others_unchanged("small")


@pytest.mark.parametrize("name", sorted(tagl1lrsuite.SHAPES))
def test_shapes(name):
    tagl1lrsuite.check_shape(name)


def test_round_trip_fill_tags_equals_the_cpu_oracle():
    tagl1lrsuite.check_round_trip()


def test_flag_and_errors():
    tagl1lrsuite.check_errors()
