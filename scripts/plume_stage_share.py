"""The share of the k_eqn and e_eqn stages in the LAST time step of a rocprofv3 kernel trace of the compiled plume step with the kEqn
model on and h assembled apart from the species (scripts/plume_keqn_timing.py <root> trace ...; fused form, single block).
usage: plume_stage_share.py <..._kernel_trace.csv>
The stages are told apart by the kernels around them, in launch order:
  step    from the last k_rho_eqn that is not the one inside a pressure corrector, i.e. the first kernel after the previous step's last
  e_eqn   after the species' tail pass (the last lambda of species_eqns) up to standin_thermo's pass
  k_eqn   after the second k_pc_finish up to correct_nut's patch pass
Prints wall time (first start to last end), summed kernel time and the kernels of each of the two stages."""
import collections
import csv
import sys

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
last = lambda sub, hi=None: max(i for i, r in enumerate(rows[:hi]) if sub in r[2])
iEnd = last("correct_nut(")                     # the step's last kernel but one (rho = psi*p follows)
iK0 = last("k_pc_finish", iEnd) + 1
iThermo = last("standin_thermo", iK0)
iE0 = last("species_eqns(", iThermo) + 1
iStep = last("k_rho_eqn", iE0)


def report(name, a, b):
    seg = rows[a:b]
    wall, busy = seg[-1][1] - seg[0][0], sum(e - s for s, e, _ in seg)
    print("%-6s %5d kernels, wall %8.3f ms, kernel time %8.3f ms" % (name, len(seg), wall / 1e6, busy / 1e6))
    return seg


report("step", iStep, iEnd + 2)
for name, a, b in (("e_eqn", iE0, iThermo), ("k_eqn", iK0, iEnd + 1)):
    seg = report(name, a, b)
    tot, cnt = collections.Counter(), collections.Counter()
    for s, e, n in seg:
        tot[n] += e - s; cnt[n] += 1
    for n, t in tot.most_common(12):
        print("    %8.3f ms %5d x  %s" % (t / 1e6, cnt[n], n[:120]))
