"""CPU: the list-scheduling model of profiles/sched_model.py and the class function of the tracer backward's longest-first order
(envgs_amd.tracing.bwd_order_class, include/envgs_trace.h: bwd_order) agree, and the model behaves on counts it can be checked on by hand."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    spec = importlib.util.spec_from_file_location("sched_model", os.path.join(ROOT, "profiles", "sched_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_class_order_is_the_library_order():
    from envgs_amd import tracing
    m = _model()
    counts = np.random.default_rng(3).integers(0, 900, 5000)
    for k in (1, 8, 32, 1024):
        order = m.class_order(counts, k)
        cls = tracing.bwd_order_class(counts, k)[order]
        assert np.array_equal(np.sort(order), np.arange(counts.size))
        assert (np.diff(cls) <= 0).all() and (np.diff(order)[np.diff(cls) == 0] > 0).all()
    assert np.array_equal(m.class_order(counts, 1), np.arange(counts.size))
    assert (np.diff(counts[m.class_order(counts, 0)]) <= 0).all()


def test_makespan_on_hand_checked_cases():
    m = _model()
    assert m.makespan(np.ones(64), slots=64) == 1.0                      # one round
    assert m.makespan(np.ones(65), slots=64) == 2.0                      # one workgroup too many
    c = np.ones(128); c[-1] = 10.0                                       # the long item last: it starts in the second round
    assert m.makespan(c, slots=64) == 11.0
    assert m.makespan(c[m.class_order(c.astype(np.int64), 0)], slots=64) == 10.0
    assert m.strided_workgroups(np.arange(10.0), grid=4).tolist() == [0 + 4 + 8, 1 + 5 + 9, 2 + 6, 3 + 7]
    r = m.report(np.stack([np.arange(1, 4097), np.zeros(4096, dtype=np.int64)], 1))
    assert r["batches"] == 4096 and r["max"] == 4096 and "makespan" in m.format_report(r)
