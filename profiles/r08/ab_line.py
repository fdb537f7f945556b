"""One line of an A/B record from bench.py's JSON on stdin: profiles/r08/ab_line.py <arm> <rep>"""
import json, sys
d = json.loads(sys.stdin.read().strip().splitlines()[-1])
sh = d.get("shapes") or {}
b = d.get("batch") or {}
g = lambda k: (sh.get(k) or {}).get("mean_launch_ms", float("nan"))
print("%-7s rep %s  cfg1 %.4f ms  value %.4e/s  ms_per_step %.3f | irregular %.4f ms | n100 %.4f n200 %.4f | "
      "64-TOI step %s ms | lnZ_checksum %.15g"
      % (sys.argv[1], sys.argv[2], d["roofline"]["mean_launch_ms"], d["value"], d["ms_per_step"], g("n2000_irregular"),
         g("n100"), g("n200"), ("%.2f" % b["ms_per_step"]) if "ms_per_step" in b else "-", d["lnZ_checksum"]))
