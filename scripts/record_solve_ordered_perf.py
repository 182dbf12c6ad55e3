"""Writes tests/golden/solve_ordered_perf.json: the bit patterns (float.hex) of initialResidual and finalResidual of
ffm_solve_ordered_d and ffm_solve_triangular_rows_d on the cases of tests/test_solve_ordered_gpu.py (perf_records there).

  python scripts/record_solve_ordered_perf.py            # needs the GPU; run it on the PARENT of a change to these solves

The test then holds the change to the parent's records, bit for bit.  Recording from the change itself proves nothing."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if __name__ == "__main__":
    from ffm_import import ffm
    from oracle import oracle as O
    import test_solve_ordered_gpu as T
    ctx = ffm.Context(0)
    records = T.perf_records(ffm, O, ctx)
    ctx.close()
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        commit = os.environ.get("FFM_RECORD_COMMIT", "unknown")
    out = dict(recorded_from=commit, device="MI355X", records=records)
    with open(T.PERF_GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
