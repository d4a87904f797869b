"""The one host pipeline behind run_packed / fetch_packed and the streams calls (Engine::run_output, finish_last_run over an
OutputPlan), on the CPU model of the kernels; test_gpu_output_plan.py runs the same cases on the MI355X.  The cases, the recorded
launch table and what each owes: tests/output_plan_cases.py."""
import pytest

import output_plan_cases as OP

from mimic3_amd._native import Engine
from tests.test_packed_streams import _blob


@pytest.fixture
def engine(emu_lib):
    cfg, blob = _blob()
    eng = Engine(blob, library=emu_lib)
    yield eng, cfg
    eng.close()


def test_each_call_launches_what_it_did_before_the_pipelines_were_one(engine):
    OP.check_launches(*engine)


def test_a_failing_late_path_serves_no_result(engine):
    OP.check_failing_late_path_serves_nothing(*engine)


def test_single_calls_replace_the_edge_cache_and_streams_calls_add_to_it(engine):
    OP.check_edge_cache(*engine)
