"""Reduce a GS_PARITY_REPORT file (tests/parity_report.py) to the DESIGN.md parity table: per test
(parametrisations folded) and tensor group, the bound asserted and the measured maxima.
usage: python tools/parity_table.py [--fold-bounds] parity.jsonl > profiles/rNN_parity_table.md
--fold-bounds: one row per test and tensor where the bound is computed per case (the conditioning rule:
frac = (4 max|ref f32 - f64| + 1e-5 max|f64|) / max|f64|); the bound column then shows the range of frac."""
import collections
import json
import re
import sys

CHAIN = {"dmeans3D", "dscales", "drotations", "dcov3D", "dmeans2D"}
FOLD = "--fold-bounds" in sys.argv[1:]
PATH = [a for a in sys.argv[1:] if not a.startswith("--")][0]
rows = collections.OrderedDict()
for line in open(PATH):
    r = json.loads(line)
    test = re.sub(r"\[.*\]$", "", r["test"])  # fold the parametrisations
    tensor = r["tensor"].split(" (")[0]
    group = "image" if tensor in ("image", "color") else ("chain" if tensor in CHAIN else "other")
    key = (test, tensor, r["rtol"], None if FOLD else r["frac"])
    a = rows.setdefault(key, dict(n=0, frac=0.0, used=0.0, lo=r["frac"], hi=r["frac"]))
    a["n"] += 1
    a["lo"], a["hi"] = min(a["lo"], r["frac"]), max(a["hi"], r["frac"])
    a["frac"] = max(a["frac"], r["max_d_over_max_ref"])
    a["used"] = max(a["used"], r["used"])
print("| test | tensor | bound: rtol·|ref| + frac·max|ref| | checks | measured max|d|/max|ref| | largest share of the bound |")
print("|---|---|---|---|---|---|")
for (test, tensor, rtol, frac), a in rows.items():
    bound = f"{a['lo']:g}" if a["lo"] == a["hi"] else f"{a['lo']:.2g} .. {a['hi']:.2g}"
    print(f"| `{test.split('::')[-1]}` ({test.split('::')[0].split('/')[-1]}) | {tensor} | {rtol:g} · {bound} | {a['n']} | "
          f"{a['frac']:.2e} | {a['used']:.2f} |")
