cd $GRAFT_REPO_ROOT
O=${OUT:-.}
python -m pytest tests/ -x -q -m gpu > $O/r5_driver_cmd.log 2>&1; echo "pytest rc=$?" | tee -a $O/r5_driver_cmd.log
python -c "import __graft_entry__ as g; g.smoke()" > $O/r5_smoke.log 2>&1; echo "smoke rc=$?"
timeout 300 python bench.py --full > $O/bench_envgs_final.json 2> $O/bench_envgs_final.err; echo "bench rc=$?"
grep -n "passed\|failed" $O/r5_driver_cmd.log | tail -2
