"""Summary of one tools/gpu_tf_iter.sh run (its outputs under $OUT, default build/iter): tests, step time, the per-phase
`kernels` of the bench line (a `--full` run), and the trace lines matching the given patterns."""
import json, os, sys
O = os.environ.get("OUT", os.path.join("build", "iter"))
print(open(os.path.join(O, "pytest_tf.txt")).read().strip())
d = json.loads(open(os.path.join(O, "bench_tf.json")).read().strip().splitlines()[-1])
print("ms/step", round(d["ms_per_step"], 3), "parts/s", round(d["value"]), "loss", d["final_loss"])
for k, v in d["kernels"].items():
    print("   ", k, round(v["avg_ms"], 4), v["launches"])
pat = sys.argv[1:] or ["steps="]
for line in open(os.path.join(O, "trace_tf.txt")):
    if any(p in line for p in pat):
        print(line.rstrip()[:150])
