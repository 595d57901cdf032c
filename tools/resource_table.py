#!/usr/bin/env python3
"""Tabulate hipcc's -Rpass-analysis=kernel-resource-usage remarks (make -C csrc asm-ppo 2> file).

    resource_table.py REMARKS [--match ppo_rows,ppo_act]          one markdown table
    resource_table.py REMARKS --against OTHER [--match ...]       also compare: exit 1 when a
                                                                  kernel of OTHER is missing or
                                                                  differs in any column
"""
import argparse
import re
import subprocess
import sys

COLS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
        "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill")
HEAD = ("VGPR", "AGPR", "SGPR", "scratch", "LDS", "occupancy", "SGPR spill", "VGPR spill")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True,
                             check=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return list(names)
    short = []
    for n in out:
        n = n.replace("(anonymous namespace)::", "")
        n = re.sub(r"^void ", "", n)
        short.append(n.split("(")[0])
    return short


def parse(path):
    rows, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = list(rows)
    return dict(zip(demangle(names), (rows[n] for n in names)))


def table(rows):
    out = ["| kernel | " + " | ".join(HEAD) + " |", "|---|" + "---|" * len(HEAD)]
    for k in sorted(rows):
        out.append(f"| `{k}` | " + " | ".join(rows[k].get(c, "?") for c in COLS) + " |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("remarks")
    ap.add_argument("--against")
    ap.add_argument("--match", default="")
    a = ap.parse_args()
    keys = [k for k in a.match.split(",") if k]
    pick = lambda rows: {k: v for k, v in rows.items() if not keys or any(s in k for s in keys)}
    mine = pick(parse(a.remarks))
    print(table(mine))
    if not a.against:
        return 0
    other = pick(parse(a.against))
    bad = [k for k in other if mine.get(k) != other[k]]
    print(f"\n{len(other)} kernels of {a.against}: {len(other) - len(bad)} identical, "
          f"{len(bad)} differ or are missing; {len(set(mine) - set(other))} new")
    for k in bad:
        print("DIFF", k, other[k], mine.get(k))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
