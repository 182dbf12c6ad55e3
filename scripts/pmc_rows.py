"""rows of every k_tile* kernel of the last step (all of them, not the 40 longest).  usage: pmc_rows.py fetch.csv write.csv nCells"""
import csv, sys, collections
def load(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], float(r["Counter_Value"])))
    rows.sort()
    return rows
def last_step(rows):
    marker = "u_eqn(ffm_plume*)::{lambda(long)#1}"
    starts = [i for i, r in enumerate(rows) if marker in r[2]]
    return rows[starts[-1]:] if starts else rows
fe, wr = load(sys.argv[1]), load(sys.argv[2]); N = int(sys.argv[3])
cal = [r[3] for r in fe if "k_reduce1<0>" in r[2]]
scale = (8.0 * N / 1024.0) / (sum(cal[-3:]) / len(cal[-3:]))
agg = collections.OrderedDict()
for rows, key in ((last_step(fe), "f"), (last_step(wr), "w")):
    for s, e, n, v in rows:
        a = agg.setdefault(n, {"f": 0.0, "w": 0.0, "nf": 0, "nw": 0, "t": 0})
        a[key] += v; a["n" + key] += 1
        if key == "f": a["t"] += e - s
print("calibration %.3f" % scale)
for n, a in agg.items():
    if "k_tile" not in n or not a["nf"]: continue
    rd = a["f"] * scale * 1024 / 1e9; wt = a["w"] * 1024 / 1e9 * (a["nf"] / max(a["nw"], 1))
    print("%-60s %5d read %8.3f write %8.3f GB/call %7.3f us/call %8.1f" % (n.replace("void ", "")[:60], a["nf"], rd / a["nf"], wt / a["nf"], (rd + wt) / a["nf"], a["t"] / a["nf"] / 1e3))
