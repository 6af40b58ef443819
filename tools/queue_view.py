#!/usr/bin/env python3
"""Which of the library's streams ran on which hardware queue, from a tools/pipe_trace.sh kernel trace of a pipelined `fast`
context: per queue the streams it carried, per stream its chain (named after the kernels it ran), dispatches and busy time per
frame.  Kernels of streams that share a queue run one after the other, so the last lines say which queues carry
more than one of the library's streams.   usage: queue_view.py <run_kernel_trace.csv> [frames = 100] [frames skipped at the end = 16]"""
import csv
import sys
from collections import defaultdict

CHAINS = [   # first match wins
    ("xlong", ("k_apply_xlong", "k_xl_")),
    ("long", ("k_apply_long", "k_long_")),
    ("T", ("k_apply", "k_find_long", "k_init_tiles", "k_rs_pass<unsigned long, false", "k_rs_hist<unsigned long")),
    ("A", ("k_points_", "k_dedup", "k_rs_pass<unsigned int", "k_rs_hist<unsigned int", "k_bundles", "k_bo_")),
    ("B", ("k_test", "k_eo2_", "k_set_params", "k_scan_local", "k_emit", "k_publish", "k_rs_pass_b", "k_rs_hist_b", "k_seed", "k_march")),
]


def short(name):
    return name.split("(")[0].replace("void ", "").replace("ksk::", "").replace("ksrs::", "")


def chain_of(name):
    s = short(name)
    for chain, keys in CHAINS:
        if any(s.startswith(k) for k in keys):
            return chain
    return "?"


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    nf = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    skip = int(sys.argv[3]) if len(sys.argv) > 3 else 16   # (the last frames' tails run in the flush, not in steady state)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(rows) if "k_points_" in r["Kernel_Name"]]
    nf = min(nf, len(idx) - skip - 1)
    start, end = idx[-skip - 1 - nf], idx[-skip - 1]
    seg = rows[start:end]
    t0, t1 = int(seg[0]["Start_Timestamp"]), int(rows[end]["Start_Timestamp"])
    has_stream = "Stream_Id" in rows[0]
    print(f"# {nf} frames, frame period {(t1 - t0) / 1e3 / nf:.1f} us (under the tracer); streams told apart by "
          + ("the trace's Stream_Id" if has_stream else "the chain their kernels belong to (no Stream_Id in this trace)"))
    # stream -> queue, chain -> busy
    busy = defaultdict(float)
    count = defaultdict(int)
    chains = defaultdict(lambda: defaultdict(float))
    top = defaultdict(lambda: defaultdict(float))
    for r in seg:
        d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        c = chain_of(r["Kernel_Name"])
        key = (r["Queue_Id"], r["Stream_Id"] if has_stream else c)
        busy[key] += d
        count[key] += 1
        chains[key][c] += d
        top[key][short(r["Kernel_Name"])[:24]] += d
    label = {}
    for key in busy:
        known = {c: v for c, v in chains[key].items() if c != "?"}
        label[key] = max(known, key=known.get) if known else "other"
    queues = sorted({k[0] for k in busy})
    shared = []
    for q in queues:
        keys = sorted((k for k in busy if k[0] == q), key=lambda k: -busy[k])
        lib = [k for k in keys if label[k] != "other"]
        qb = sum(busy[k] for k in keys)
        print(f"queue {q}: {len(lib)} library stream(s), kernels executing {qb / nf:.0f} us/frame = {100 * qb * 1e3 / (t1 - t0):.0f} % of the time")
        for k in keys:
            kern = ", ".join(f"{n} {v / nf:.0f}" for n, v in sorted(top[k].items(), key=lambda kv: -kv[1])[:4])
            print(f"    stream {k[1]:>5}  stage {label[k]:<5}  {count[k] / nf:5.1f} dispatches/frame  {busy[k] / nf:6.1f} us/frame   {kern}")
        if len(lib) > 1:
            shared.append((q, [label[k] for k in lib]))
    nlib = sum(1 for k in busy if label[k] != "other")
    print(f"# library streams seen: {nlib} on {len(queues)} hardware queue(s)")
    if shared:
        for q, ls in shared:
            print(f"# queue {q} carries {len(ls)} library streams: {' + '.join(ls)}")
    else:
        print("# no two library streams share a hardware queue")


if __name__ == "__main__":
    main()
