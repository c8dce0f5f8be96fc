"""The tag trainer on the MI355X against the restatement of tests/tagtrainref.py (the checks of tests/tagtrainsuite.py), and the round
trip: a model trained on a corpus whose tags an adjacent char decides, loaded with predict_tags, evaluated against its training corpus."""
import numpy as np
import pytest

from tests import tagtrainsuite
from vaporetto_amd import api

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(tagtrainsuite.CASES))
def test_problems_match_restatement(name):
    tagtrainsuite.check_problems(name)


@pytest.mark.parametrize("solver", [0, 2])
@pytest.mark.parametrize("name", sorted(tagtrainsuite.CASES))
def test_solver_model_and_determinism(name, solver):
    _, stats = tagtrainsuite.check_solver(name, solver)
    paths = {p["path"] for p in stats["problems"]}
    assert paths == ({1, 2} if name == "large" else {1})


@pytest.mark.parametrize("solver", [0, 2])
def test_every_problem_through_the_global_memory_solver(solver):
    _, stats = tagtrainsuite.check_solver("small", solver, path=1)
    assert {p["path"] for p in stats["problems"]} == {2}


# a problem exactly at the in-kernel solver's limit of 7 * (features + 1) + 3 * rows = 7424 doubles of LDS, and one double past it
@pytest.mark.parametrize("total,path", [(7424, 1), (7425, 2)])
def test_problem_at_the_lds_limit(total, path):
    tagtrainsuite.check_limit(total, path)


def test_flag_and_errors():
    tagtrainsuite.check_errors()


def test_round_trip_reproduces_every_gold_tag():
    tagtrainsuite.check_round_trip()


@pytest.mark.parametrize("name", ["small", "large", "decided"])
def test_writer_and_evaluate_equal_the_cpu_oracle_on_the_trained_model(name):
    tagtrainsuite.check_oracle_round_trip(name)
