"""The tag trainer's kernels and host driver on the CPU emulator (tests/native/hipemu) against the restatement of tests/tagtrainref.py:
the problem list, keys, CSR and y; both solver paths; the model bytes and determinism; the flag and the errors."""
import numpy as np
import pytest

from tests import emu, tagtrainsuite
from vaporetto_amd import _lib, api


@pytest.fixture(scope="module", autouse=True)
def emulated():
    saved = _lib._lib
    _lib._lib = emu.load()
    yield
    _lib._lib = saved


@pytest.mark.parametrize("name", sorted(tagtrainsuite.CASES))
def test_problems_match_restatement(name):
    tagtrainsuite.check_problems(name)


@pytest.mark.parametrize("name,solver", [("small", 0), ("small", 2), ("large", 0), ("large", 2)])
def test_solver_model_and_determinism(name, solver):
    _, stats = tagtrainsuite.check_solver(name, solver)
    paths = {p["path"] for p in stats["problems"]}
    assert paths == ({1, 2} if name == "large" else {1})


def test_every_problem_through_the_global_memory_solver():
    _, stats = tagtrainsuite.check_solver("small", 2, path=1)
    assert {p["path"] for p in stats["problems"]} == {2}


# a problem exactly at the in-kernel solver's limit of 7 * (features + 1) + 3 * rows = 7424 doubles of LDS, and one double past it
@pytest.mark.parametrize("total,path", [(7424, 1), (7425, 2)])
def test_problem_at_the_lds_limit(total, path):
    tagtrainsuite.check_limit(total, path)


def test_flag_and_errors():
    tagtrainsuite.check_errors()
