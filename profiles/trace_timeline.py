"""Kernel timeline from `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py ...`.

usage: python3 profiles/trace_timeline.py DIR [START [COUNT]]
       python3 profiles/trace_timeline.py DIR tail
       python3 profiles/trace_timeline.py DIR ends
START: index into the list of k_sweep_cluster launches (negative counts from the end) at which to begin, or the word
`run` to begin at the k_init_samples launch of the 3rd complete run; COUNT: rows to print (default 40).
`tail`: the critical path between two sweep kernels of one run -- from the end of a k_sweep_cluster launch to the start of the
next one, split into the kernels of the same queue in between (what runs on the quadrature's stream, beside the next sweep, is left
out) and the gaps in front of each of them and of the next sweep kernel; medians over all such pairs of the trace, in us.
`ends`: the two ends of a run around its sweep kernels, with the kernels of BOTH queues -- the head from the start of k_reset to the
start of the first k_sweep_cluster, and the end from the finish of the last k_sweep_cluster that sweeps to the finish of the run's
last kernel (a kernel trace holds no copies: the copy behind the last kernel is not in it; the distance to the next run's k_reset,
which holds that copy and the host's work between two runs, is printed beside it).  Medians over the runs of the trace that
launch the same kernels in the same order, in us; every kernel with its queue, its start and its end relative to the segment."""
import csv
import glob
import statistics
import sys

f = glob.glob(sys.argv[1] + '/**/*kernel_trace.csv', recursive=True)[0]
rows = list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r['Start_Timestamp']))
start = sys.argv[2] if len(sys.argv) > 2 else "20"
count = int(sys.argv[3]) if len(sys.argv) > 3 else 40


def short(name):
    return name.split('(')[0].replace('void ', '')[:40]


if start == "tail":
    med = statistics.median
    sw = [i for i, r in enumerate(rows) if 'k_sweep_cluster' in r['Kernel_Name']]
    pairs = []          # (end-to-start, kernel time, gap time, ((name, gap in front, duration), ...), gap in front of the next sweep kernel)
    for a, b in zip(sw, sw[1:]):
        mid = [r for r in rows[a + 1:b] if r['Queue_Id'] == rows[a]['Queue_Id']]      # the main stream's queue
        if any(k in r['Kernel_Name'] for r in mid for k in ('k_reset', 'k_init', 'k_fin_')):
            continue    # the next run's first sweep kernel: not a pair of one run
        t = int(rows[a]['End_Timestamp'])
        steps = []
        for r in mid:
            s, e = int(r['Start_Timestamp']), int(r['End_Timestamp'])
            steps.append((short(r['Kernel_Name']), (s - t) / 1e3, (e - s) / 1e3))
            t = max(t, e)
        last = (int(rows[b]['Start_Timestamp']) - t) / 1e3
        ktime = sum(x[2] for x in steps)
        e2s = (int(rows[b]['Start_Timestamp']) - int(rows[a]['End_Timestamp'])) / 1e3
        pairs.append((e2s, ktime, e2s - ktime, tuple(steps), last))
    # the speculative launch behind the last sweep exits on the stop flag: a pair in front of it counts like any other
    shapes = {}
    for p in pairs:
        shapes.setdefault(tuple(x[0] for x in p[3]), []).append(p)
    sweeps = [(int(rows[i]['End_Timestamp']) - int(rows[i]['Start_Timestamp'])) / 1e3 for i in sw]
    real = [x for x in sweeps if x > 20.0]
    print(f"k_sweep_cluster: {len(real)} launches that sweep, median {med(real):.1f} us (min {min(real):.1f}, max {max(real):.1f}); "
          f"{len(sweeps) - len(real)} that exit on the stop flag")
    for names, ps in sorted(shapes.items(), key=lambda kv: -len(kv[1])):
        print(f"{len(ps)} pairs with {len(names)} launches in between: end-to-start median {med(p[0] for p in ps):.1f} us "
              f"(min {min(p[0] for p in ps):.1f}, max {max(p[0] for p in ps):.1f}) = kernels {med(p[1] for p in ps):.1f} + gaps {med(p[2] for p in ps):.1f}")
        for k, nm in enumerate(names):
            print(f"    gap {med(p[3][k][1] for p in ps):6.1f}  dur {med(p[3][k][2] for p in ps):6.1f}  {nm}")
        print(f"    gap {med(p[4] for p in ps):6.1f}  k_sweep_cluster (next)")
    sys.exit(0)
if start == "ends":
    med = statistics.median
    resets = [i for i, r in enumerate(rows) if 'k_reset' in r['Kernel_Name']]
    heads, tails = {}, {}
    for a, b in zip(resets, resets[1:]):
        run = rows[a:b]
        sw = [i for i, r in enumerate(run) if 'k_sweep_cluster' in r['Kernel_Name']]
        real = [i for i in sw if int(run[i]['End_Timestamp']) - int(run[i]['Start_Timestamp']) > 20000]
        if not real:
            continue
        main = run[0]['Queue_Id']
        q = lambda r: 'main' if r['Queue_Id'] == main else 'side'
        t0 = int(run[0]['Start_Timestamp'])
        seg = [(q(r), short(r['Kernel_Name']), (int(r['Start_Timestamp']) - t0) / 1e3, (int(r['End_Timestamp']) - t0) / 1e3) for r in run[:sw[0]]]
        seg.append(('main', 'k_sweep_cluster (first) starts', (int(run[sw[0]]['Start_Timestamp']) - t0) / 1e3, (int(run[sw[0]]['Start_Timestamp']) - t0) / 1e3))
        heads.setdefault(tuple(x[:2] for x in seg), []).append(seg)
        t1 = int(run[real[-1]]['End_Timestamp'])
        rest = [r for r in run[real[-1] + 1:] if int(r['End_Timestamp']) > t1]
        seg = [(q(r), short(r['Kernel_Name']), (int(r['Start_Timestamp']) - t1) / 1e3, (int(r['End_Timestamp']) - t1) / 1e3) for r in rest]
        seg.append(('main', 'k_reset (next run) starts', (int(rows[b]['Start_Timestamp']) - t1) / 1e3, (int(rows[b]['Start_Timestamp']) - t1) / 1e3))
        tails.setdefault(tuple(x[:2] for x in seg), []).append(seg)
    for title, shapes in (("head: start of k_reset -> start of the first k_sweep_cluster", heads),
                          ("end: finish of the last sweeping k_sweep_cluster -> finish of the last kernel", tails)):
        for names, segs in sorted(shapes.items(), key=lambda kv: -len(kv[1]))[:2]:
            total = [max(x[3] for x in s[:-1]) if len(s) > 1 else 0.0 for s in segs] if title[0] == 'e' else [s[-1][3] for s in segs]
            print(f"{title}: {len(segs)} runs, median {med(total):.1f} us (min {min(total):.1f}, max {max(total):.1f})")
            busy = {'main': 0.0, 'side': 0.0}
            for k, (qq, nm) in enumerate(names):
                st_, en_ = med(s[k][2] for s in segs), med(s[k][3] for s in segs)
                gap = st_ - busy[qq]
                busy[qq] = max(busy[qq], en_)
                print(f"    {qq}  start {st_:7.1f}  end {en_:7.1f}  dur {med(s[k][3] - s[k][2] for s in segs):6.1f}  gap on its queue {gap:6.1f}  {nm}")
    sys.exit(0)
if start == "run":
    inits = [i for i, r in enumerate(rows) if 'k_init_samples' in r['Kernel_Name']]
    i0 = inits[2] - 8
else:
    idx = [i for i, r in enumerate(rows) if 'k_sweep_cluster' in r['Kernel_Name']]
    i0 = idx[int(start)]
t0 = int(rows[i0]['Start_Timestamp'])
prev_end = t0
for r in rows[i0:i0 + count]:
    s, e = int(r['Start_Timestamp']), int(r['End_Timestamp'])
    print(f"{(s - t0) / 1e3:9.1f} us  gap {(s - prev_end) / 1e3:6.1f}  dur {(e - s) / 1e3:7.1f}  {r['Kernel_Name'][:60]}")
    prev_end = max(prev_end, e)
