"""From a rocprofv3 --kernel-trace csv of `python bench.py`: inside the densest 300 ms window of k_bow_topk launches (the timed
steps), summed kernel time / wall, the greatest number of kernels running at one instant, the distinct queues, the share of
wall time by number of kernels running, and K5's rounds per query (working rounds, launches that found the state finished,
queries that came back for more rounds).  usage: trace_concurrency.py trace.csv"""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
marks = sorted(int(r["Start_Timestamp"]) for r in rows if "k_bow_topk" in r["Kernel_Name"])
win = 300e6
best, j = (0, 0), 0
for i, t in enumerate(marks):
    while marks[j] < t - win:
        j += 1
    if i - j + 1 > best[0]:
        best = (i - j + 1, j)
a = marks[best[1]]
b = a + win
pts = []
queues = set()
for r in rows:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    if e <= a or s >= b:
        continue
    pts.append((max(s, a), 1))
    pts.append((min(e, b), -1))
    queues.add(r.get("Queue_Id"))
pts.sort(key=lambda p: (p[0], p[1]))
conc = peak = 0
area = 0
last = a
hist = {}
for t, d in pts:
    area += conc * (t - last)
    hist[conc] = hist.get(conc, 0) + (t - last)
    last = t
    conc += d
    peak = max(peak, conc)
print(f"window 300 ms, {best[0]} queries: summed kernel time / wall = {area / win:.2f}; greatest number of kernels "
      f"running at one instant = {peak}; distinct queues in the window = {len(queues)}")
rounds = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows
          if "k_p3p_round" in r["Kernel_Name"] and a <= int(r["Start_Timestamp"]) < b]
fin = sum(1 for r in rows if "k_p3p_finish" in r["Kernel_Name"] and a <= int(r["Start_Timestamp"]) < b)
nq = best[0]
noop = sum(1 for d in rounds if d < 6000)
work = [d for d in rounds if d >= 6000]
print(f"K5 per query: {len(rounds) / nq:.2f} round launches, of which {noop / nq:.2f} shorter than 6 us (queued past the end: "
      f"no-ops) and {len(work) / nq:.2f} working rounds of {sum(work) / max(1, len(work)) / 1e3:.1f} us mean; "
      f"{fin / nq:.3f} k_p3p_finish launches (share of queries that came back for more rounds: {fin / nq - 1:.3f})")
print("share of wall time by number of kernels running:",
      ", ".join(f"{k}: {100 * v / win:.1f} %" for k, v in sorted(hist.items())))
