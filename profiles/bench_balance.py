"""bench.py under a value of the ENVGS_DBG_BALANCE switch (include/envgs_raster.h), for the round-7 A/B inside one build:

    python profiles/bench_balance.py VALUE [bench.py arguments]

VALUE bit 1 = the record backward's batches in coherence order over the capped grid (the dispatch until round 7); VALUE >> 8 = classes K of the
longest-first order (0 = default).  bench.py itself sets the switches it knows and leaves this one alone."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:] = [ROOT] + [p for p in sys.path if os.path.abspath(p or ".") != os.path.dirname(os.path.abspath(__file__))]
value = int(sys.argv[1])
from envgs_amd import _lib  # noqa: E402

for kind in (("product", "diag") if "--diag" in sys.argv else ("product",)):
    old = _lib.select(kind)
    _lib.load().envgs_debug_set(6, value)
    _lib.select(old)
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[2:]
runpy.run_path(sys.argv[0], run_name="__main__")
