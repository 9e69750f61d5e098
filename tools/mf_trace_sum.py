"""Visit-weighted means of the [async visit], [async push], relabel-visit and [dense push visits] lines of GGC_MF_TRACE logs
(the dense push visits of a solve's first round and of its later rounds apart):
   GGC_MF_TRACE=1 python3 tools/mf_trace.py 2> LOG; python3 tools/mf_trace_sum.py LOG ..."""
import re
import sys

for path in sys.argv[1:]:
    L = open(path).read().splitlines()
    n = 0; acc = [0.0] * 8; launches = 0; alive = 0.0; foll = 0; cut = 0; idle = 0; high = 0; hop_launches = 0
    pend = None
    for l in L:
        m = re.search(r"\[async visit\] load\+fill ([\d.]+) us, sweeps ([\d.]+) us \(([\d.]+) sweeps\), write-back\+drain ([\d.]+)", l)
        if m: pend = [float(x) for x in m.groups()]; continue
        m = re.search(r"\[async push\] (\d+) waves alive ([\d.]+) us on average; (\d+) visits \((\d+) followed\): per visit wait\+lock ([\d.]+) us, visit ([\d.]+) us, hand-over ([\d.]+)", l)
        if m and pend:
            c = re.search(r"chains cut by the hop limit (\d+), ended with nothing to hand on (\d+), highest label written (\d+)", l)
            if c: cut += int(c.group(1)); idle += int(c.group(2)); high = max(high, int(c.group(3))); hop_launches += int(c.group(1)) > 0
            v = int(m.group(3)); n += v; launches += 1; foll += int(m.group(4)); alive += float(m.group(2))
            for i, x in enumerate(pend + [float(m.group(5)), float(m.group(6)), float(m.group(7))]): acc[i] += x * v
            pend = None
    if n:
        a = [x / n for x in acc]
        print(f"{path}: push launches {launches}, visits {n} ({foll} followed), waves alive {alive / launches:.1f} us/launch mean; per visit: "
              f"load+fill {a[0]:.2f}, sweeps {a[1]:.2f} ({a[2]:.2f} sweeps, {a[1] / max(a[2], 1e-9):.3f} us each), write-back+drain {a[3]:.2f}, "
              f"wait+lock {a[4]:.2f}, visit {a[5]:.2f}, hand-over {a[6]:.2f}")
        print(f"   [chains] cut by the hop limit {cut} (in {hop_launches} of {launches} launches), ended with nothing to hand on {idle}, highest label written {high}")
    # the label ceiling: lmax over the rounds' open images, and the excess it parked against what the next relabel found reachable
    rounds = 0; lo = None; hi = 0; mean = 0.0; parked = 0; wrong = 0; wrong_rounds = 0
    for l in L:
        m = re.search(r"\[ceiling\] slack (-?\d+), lmax of (\d+) open images: min (\d+), mean ([\d.]+), max (\d+); parked pixels with excess (\d+), of them finite after the relabel (\d+)", l)
        if m and int(m.group(2)):
            rounds += 1; lo = int(m.group(3)) if lo is None else min(lo, int(m.group(3))); hi = max(hi, int(m.group(5))); mean += float(m.group(4))
            parked += int(m.group(6)); wrong += int(m.group(7)); wrong_rounds += int(m.group(7)) > 0
    if rounds:
        print(f"   [ceiling] {rounds} rounds with open images: lmax min {lo}, mean of the rounds' means {mean / rounds:.1f}, max {hi}; parked pixels with excess "
              f"{parked}, of them finite after the relabel {wrong} ({wrong / rounds:.2f} per round, in {wrong_rounds} rounds)")
    for tag in ("async relabel visits", "relabel visits"):
        n = 0; acc = [0.0] * 6
        for l in L:
            m = re.search(r"\[" + tag + r"\] (\d+) \w+ visits: per visit load\+fill ([\d.]+) us, sweeps ([\d.]+) us \(([\d.]+) sweeps, ([\d.]+) BFS levels, (\d+) visits fell back\), write-back ([\d.]+)", l)
            if m:
                v = int(m.group(1)); n += v
                for i, x in enumerate([float(m.group(k)) for k in (2, 3, 4, 5, 7)]): acc[i] += x * v
                acc[5] += int(m.group(6))
        if n:
            a = [x / n for x in acc[:5]]
            print(f"   [{tag}] {n} visits: load+fill {a[0]:.2f}, sweeps|levels {a[1]:.2f} ({a[2]:.2f} sweeps, {a[3]:.2f} levels, {int(acc[5])} fell back), write-back(+hand-over) {a[4]:.2f}")
    rows = {"first round": [0, [0.0] * 5], "later rounds": [0, [0.0] * 5]}
    first = True                                           # a "round 0:" line precedes the first dense push of a solve
    for l in L:
        m = re.search(r"\[ggc maxflow\] round (\d+):", l)
        if m: first = m.group(1) == "0"; continue
        m = re.search(r"\[dense push visits\] (\d+) visits: per visit load\+fill ([\d.]+) us, sweeps ([\d.]+) us \(([\d.]+) sweeps, ([\d.]+) with a deal\), write-back\+hand-over ([\d.]+)", l)
        if m:
            row = rows["first round" if first else "later rounds"]
            v = int(m.group(1)); row[0] += v
            for i in range(5): row[1][i] += float(m.group(2 + i)) * v
    for tag, (n, acc) in rows.items():
        if n:
            a = [x / n for x in acc]
            print(f"   [dense push visits, {tag}] {n} visits: load+fill {a[0]:.2f}, sweeps {a[1]:.2f} ({a[2]:.2f} sweeps, {a[1] / max(a[2], 1e-9):.3f} us each, "
                  f"{a[3]:.2f} with a deal), write-back+hand-over {a[4]:.2f}")
