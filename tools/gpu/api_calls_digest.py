"""HIP API names of a rocprofv3 --hip-trace csv, per thread in start order: names + sha256."""
import csv
import glob
import hashlib
import sys

src, out = sys.argv[1], sys.argv[2]
files = glob.glob(src + "/**/*hip_api_trace.csv", recursive=True)
assert len(files) == 1, files
rows = list(csv.DictReader(open(files[0])))
threads = {}
for r in rows:
    threads.setdefault(r["Thread_Id"], []).append((int(r["Start_Timestamp"]), r["Function"]))
order = sorted(threads, key=lambda t: min(threads[t])[0])
lines = []
for k, t in enumerate(order):
    lines.append(f"# thread {k}: {len(threads[t])} calls")
    lines += [name for _, name in sorted(threads[t])]
text = "\n".join(lines) + "\n"
open(out, "w").write(text)
print(out, len(rows), "calls", len(order), "threads", hashlib.sha256(text.encode()).hexdigest())
