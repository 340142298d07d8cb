"""Dev tool: the dispatches of the LAST compare-exchange in a rocprofv3 kernel-trace csv of tools/gpu_cx_trace.py, in order, and
their count per kernel.  A compare-exchange starts with its comparison's step 1, whose first dispatch is `k_plain_alice`.

    python tools/cx_dispatches.py kernel_trace.csv
"""
import csv
import sys
from collections import Counter

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
starts = [i for i, r in enumerate(rows) if "k_plain_alice" in r["Kernel_Name"]]
if not starts:
    sys.exit("no k_plain_alice dispatch in the trace")
last = rows[starts[-1]:]
t0 = int(last[0]["Start_Timestamp"])


def short(name):
    name = name.replace("void ", "")
    return name[:name.find("(")] if "(" in name else name


print(f"one compare-exchange: {len(last)} dispatches over {(int(last[-1]['End_Timestamp']) - t0) / 1e6:.2f} ms")
for r in last:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    print(f"  at {(s - t0) / 1e6:9.3f} ms  {(e - s) / 1e6:8.3f} ms  grid {r.get('Grid_Size', '?'):>9}  {short(r['Kernel_Name'])[:90]}")
print("\ndispatches per kernel:")
for name, n in sorted(Counter(short(r["Kernel_Name"]) for r in last).items(), key=lambda kv: (-kv[1], kv[0])):
    print(f"  {n:4d}  {name[:100]}")
