"""Device twin of tests/test_output_plan.py (pytest -m gpu): the one host pipeline behind run_packed / fetch_packed and the streams
calls on the MI355X.  The same cases and the same recorded launch table: tests/output_plan_cases.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import output_plan_cases as OP  # noqa: E402

from mimic3_amd._native import Engine  # noqa: E402
from tests.test_packed_streams import _blob  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def engine(gpu_lib):
    cfg, blob = _blob()
    eng = Engine(blob, device=0, library=gpu_lib)
    yield eng, cfg
    eng.close()


def test_each_call_launches_what_it_did_before_the_pipelines_were_one(engine):
    OP.check_launches(*engine)


def test_a_failing_late_path_serves_no_result(engine):
    OP.check_failing_late_path_serves_nothing(*engine)


def test_single_calls_replace_the_edge_cache_and_streams_calls_add_to_it(engine):
    OP.check_edge_cache(*engine)
