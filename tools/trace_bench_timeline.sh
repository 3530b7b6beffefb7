# GPU box: kernel + memory-copy timeline of a short bench run (do the copies run under the kernels?) -> gpurun_out/<tag>/timeline.txt
# Beside it: the library's kernels on the compute lane one by one with the idle time in front of each -> kernels.txt, and the gaps between the kernel classes of a batch
# (PREP -> ME -> OIS -> PACK -> next PREP; the descriptor copies in front of the launches are not counted as kernels) -> gaps.txt.  SVT_PRODUCT_LIB selects the build.
cd ${GRAFT_REPO_ROOT:-.}
export TMPDIR=/tmp
O=gpurun_out/${1:-timeline}
mkdir -p $O
timeout 300 rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d $O/tr -o t -- python bench.py --no-cpu-baseline --no-encoder-fps --no-pmc --steps 4 --warmup 2 > $O/tr.log 2>&1 < /dev/null
python - "$O" <<'PY'
import csv, glob, sys
O = sys.argv[1]
ev = []
for f in glob.glob(O + "/tr/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        n = r["Kernel_Name"]
        # a copy the runtime makes with a kernel of its own does not appear in the memory-copy trace
        tag = "PACK" if "pack" in n else "ME" if "k_me" in n else "OIS" if "ois" in n else "PREP" if "prep" in n else "COPY KERNEL (runtime)" if "copyBuffer" in n else None
        if tag:
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), tag))
for f in glob.glob(O + "/tr/**/*memory_copy_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Direction"].replace("MEMORY_COPY_", "") + " %.0fMB" % (int(r.get("Bytes", r.get("Size", 0)) or 0) / 1e6)))
ev.sort()
t0 = ev[0][0]
big = [e for e in ev if e[1] - e[0] > 200000]
with open(O + "/timeline.txt", "w") as out:
    for s, e, n in big[-70:]:
        print("%9.3f -> %9.3f ms  (%7.3f)  %s" % ((s - t0) / 1e6, (e - t0) / 1e6, (e - s) / 1e6, n), file=out)
print(open(O + "/timeline.txt").read())
# the compute lane alone: every kernel of the library, small ones included
lane = []
for f in glob.glob(O + "/tr/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        n = r["Kernel_Name"]
        tag = "PACK_ME" if "k_pack_me" in n else "PACK_OIS" if "k_pack_ois" in n else "ME" if "k_me" in n else "OIS" if "k_ois" in n else "PREP" if "prep" in n else "DESC" if "k_copy_words" in n else None
        if tag:
            lane.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), tag))
lane.sort()
with open(O + "/kernels.txt", "w") as out:
    for i, (s, e, n) in enumerate(lane[-200:]):
        gap = (s - lane[-200:][i - 1][1]) / 1e6 if i else 0.0
        print("%9.3f -> %9.3f ms  (%7.3f)  gap before %7.3f  %s" % ((s - t0) / 1e6, (e - t0) / 1e6, (e - s) / 1e6, gap, n), file=out)
main, gaps = [x for x in lane if x[2] != "DESC"], {}
for a, b in zip(main, main[1:]):
    if a[2] != b[2]:
        gaps.setdefault(a[2] + " -> " + b[2], []).append((b[0] - a[1]) / 1e6)
with open(O + "/gaps.txt", "w") as out:
    for k, v in sorted(gaps.items()):
        v = sorted(v[len(v) // 2:])  # the timed half of the run
        print("%-22s n=%3d  median %.3f  min %.3f  max %.3f ms" % (k, len(v), v[len(v) // 2], v[0], v[-1]), file=out)
print(open(O + "/gaps.txt").read())
PY
rm -rf $O/tr
