"""Kernel averages of a `rocprofv3 --kernel-trace` run of bench.py without the launches that exit at once: every solve queues one
iteration ahead of the news that it is over, and each kernel of that iteration returns after reading `term`.
Per kernel the `--solves` shortest launches are dropped (one per solve) and the rest averaged.

  python scripts/kernel_avg.py <..._kernel_trace.csv> [--solves 4] [name-substring ...]"""
import argparse
import collections
import csv

ap = argparse.ArgumentParser()
ap.add_argument("trace")
ap.add_argument("--solves", type=int, default=4)
ap.add_argument("names", nargs="*", default=["k_track_sweep_dense", "k_update_sweep", "k_reduce_slabs", "k_chol_level", "k_assemble", "k_inv_y",
                                             "k_lm_reduce_decide"])
a = ap.parse_args()
dur = collections.defaultdict(list)
with open(a.trace, newline="") as f:
    for row in csv.DictReader(f):
        dur[row["Kernel_Name"]].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
for want in a.names:
    for name, d in sorted(dur.items()):
        if want not in name:
            continue
        d = sorted(d)
        kept = d[a.solves:] if len(d) > a.solves else d
        print(f"{name.split('(')[0]:60s} launches {len(d):5d} all {sum(d) / len(d) / 1e3:9.3f} us | without the {len(d) - len(kept)} shortest "
              f"(<= {d[len(d) - len(kept) - 1] / 1e3 if len(kept) < len(d) else 0:.2f} us): {sum(kept) / len(kept) / 1e3:9.3f} us  median {kept[len(kept) // 2] / 1e3:.2f} min {kept[0] / 1e3:.2f} max {kept[-1] / 1e3:.2f}")
