"""The dispatches of one labelling (fb_fem_parts) from a kernel trace of `tools/probe_parts.py --trace`, in launch order.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/probe_parts.py --trace
    python tools/show_parts_trace.py DIR > profiles/parts_kernel_trace.txt

Reads the profiler's CSV or its default database.  Takes the last window that begins at k_parts_face_keys and ends at the last k_parts_* labelling kernel behind it; rocPRIM's passes and
the runtime's fills and copies inside the window are the labelling's own."""
import csv
import glob
import os
import sys


def short(name):
    if "rocprim" in name:
        return "rocprim pass (radix sort / select / scan)"
    name = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
    return name.replace("fb::", "").replace(" [clone .kd]", "").replace(".kd", "")


def main():
    files = sorted(glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True))
    dbs = sorted(glob.glob(os.path.join(sys.argv[1], "**", "*_results.db"), recursive=True))
    rows = []
    if files:
        for r in csv.DictReader(open(files[-1])):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    elif dbs:   # (the profiler's default output: its `kernels` view)
        import sqlite3
        for start, end, name in sqlite3.connect(dbs[-1]).execute("select start, end, name from kernels"):
            rows.append((int(start), int(end), short(name)))
    else:
        raise SystemExit("no *kernel_trace.csv or *_results.db under " + sys.argv[1])
    rows.sort()
    label = ("k_parts_face_keys", "k_parts_keys_ab", "k_parts_hook", "k_parts_flatten", "k_parts_label", "k_parts_heads", "k_parts_chunks", "k_parts_chunk_volumes",
             "k_parts_volumes", "k_parts_node_min", "k_parts_node_shared", "k_parts_node_out", "k_parts_corner_keys", "k_parts_foreign_count")
    first = max(i for i, r in enumerate(rows) if r[2] == "k_parts_face_keys")
    last = max(i for i, r in enumerate(rows) if i >= first and r[2] in label and not any(x[2] == "k_split_front" for x in rows[first:i]))
    win = rows[first:last + 1]
    total, groups = 0.0, {}
    for s, e, n in win:
        print("%8.1f us  %s" % ((e - s) / 1e3, n))
        total += (e - s) / 1e3
        groups[n] = groups.get(n, 0.0) + (e - s) / 1e3
    print("sum of device time %.1f us; first start to last end %.1f us" % (total, (win[-1][1] - win[0][0]) / 1e3))
    print("by kernel: " + "; ".join("%s %.1f us" % (n, t) for n, t in sorted(groups.items(), key=lambda x: -x[1])))


if __name__ == "__main__":
    main()
