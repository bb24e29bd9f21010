#!/usr/bin/env python3
"""Per-kernel comparison of two builds of the kernel-holding units: resources and instruction streams (the method of profiles/one_kernel_per_stage.txt).

    make -C cpu-raytracing-experiments_amd/csrc asm 2> remarks.log      (at each commit; keep the mirt_*_gfx950.s listings and the log)
    python profiles/compare_kernels.py parent.s change.s parent_remarks.log change_remarks.log [--all] [--order]

Each of the four arguments may be several files joined by commas (a side built from several units: mirt_launch_gfx950.s,mirt_resolve_gfx950.s);
kernels pair by name across the union of a side's files.  Kernels are the functions the -Rpass-analysis=kernel-resource-usage remarks name; they pair by (demangled) name.  Per kernel: the resource block
of the remarks — VGPRs, AGPRs, TotalSGPRs, VGPRs spilled, SGPRs spilled, scratch B/lane, LDS B/block, occupancy waves/SIMD — and the text between
the function's label and .Lfunc_end (the instructions and the kernel descriptor's .amdhsa_ lines) with comment lines, trailing comments and
blank lines stripped and .LBBn_m label numbers normalised.  Prints the rows that differ (--all: every row) and a summary; --order also prints where each list of kernels first differs in
the order of emission (several files on a side: each listing of the change against the parent's order of the kernels it holds).  Exit status 1 if a name is unpaired or a resource figure differs.  Host-only: plain Python, c++filt if there is one."""
import argparse
import re
import shutil
import subprocess
import sys

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void ", "", d).replace("mirt::", "")
        depth = 0
        for i, ch in enumerate(d):                      # cut the argument list: the first '(' outside <...>
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                d = d[:i]
                break
        short[n] = d
    return short


def lines_of(paths):
    for path in paths.split(","):
        yield from open(path, errors="replace")


def resources(log):
    """{mangled name: tuple of FIELDS} in the order of the remarks."""
    res, cur = {}, None
    for line in lines_of(log):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
        if m and cur:
            res[cur][m.group(1)] = m.group(2)
    return {k: tuple(v.get(f, "?") for f in FIELDS) for k, v in res.items()}


def streams(listing, kernels):
    """{mangled name: list of instruction lines}, labels normalised per function."""
    out, cur, body = {}, None, None
    for line in lines_of(listing):
        if cur is None:
            m = re.match(r"^(\S+):\s*; @\1\s*$", line)
            if m and m.group(1) in kernels:
                cur, body, labels = m.group(1), [], {}
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[cur] = body
            cur = None
            continue
        text = line.split(";", 1)[0].rstrip()
        if not text.strip():
            continue
        text = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), text)
        body.append(re.sub(r"\s+", " ", text.strip()))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_s"), ap.add_argument("change_s"), ap.add_argument("parent_log"), ap.add_argument("change_log")
    ap.add_argument("--all", action="store_true", help="print every row, not only those that differ")
    ap.add_argument("--order", action="store_true", help="print where the order of emission first differs")
    a = ap.parse_args()
    rp, rc = resources(a.parent_log), resources(a.change_log)
    sp, sc = streams(a.parent_s, rp), streams(a.change_s, rc)
    names = demangle(sorted(set(rp) | set(rc)))
    only_p, only_c = sorted(names[n] for n in set(rp) - set(rc)), sorted(names[n] for n in set(rc) - set(rp))
    width = max(len(names[n]) for n in names) + 2
    print(f"{'kernel':{width}}{'resources (parent)':32}{'resources':32}instruction stream")
    same = res_diff = stream_diff = 0
    for n in sorted(set(rp) & set(rc), key=lambda n: names[n]):
        r = "same" if rp[n] == rc[n] else "DIFF -> " + " ".join(rc[n])
        p, c = sp.get(n), sc.get(n)
        if p is None or c is None:
            s = "NOT FOUND in a listing"
        elif p == c:
            s = f"same ({len(p)} lines)"
        else:
            first = next((f"{x} | {y}" for x, y in zip(p, c) if x != y), "one is a prefix of the other")
            s = f"DIFF ({len(p)} -> {len(c)} lines; first: {first})"
        res_diff += rp[n] != rc[n]
        stream_diff += p != c
        same += rp[n] == rc[n] and p == c
        if a.all or rp[n] != rc[n] or p != c:
            print(f"{names[n]:{width}}{' '.join(rp[n]):32}{r:32}{s}")
    print(f"\n{len(rp)} kernels in the parent, {len(rc)} in the change; {len(only_p)} only in the parent, {len(only_c)} only in the change.")
    for label, lst in (("only in the parent", only_p), ("only in the change", only_c)):
        for n in lst:
            print(f"  {label}: {n}")
    print(f"{same} pairs identical in resources and instruction stream, {res_diff} with a resource difference, {stream_diff} with a stream difference.")
    if a.order:
        for listing in a.change_s.split(",") if "," in a.change_s + a.parent_s else [None]:
            held = rc if listing is None else streams(listing, rc)
            op, oc = [names[n] for n in rp if listing is None or n in held], [names[n] for n in rc if n in held]
            i = next((i for i, (x, y) in enumerate(zip(op, oc)) if x != y), None)
            print("order of emission" + ("" if listing is None else f" ({listing}, {len(oc)} kernels)") + ": "
                  + ("the same" if i is None and len(op) == len(oc) else f"first differs at position {i}: {op[i]} | {oc[i]}" if i is not None else "one list is a prefix of the other"))
    return 1 if only_p or only_c or res_diff else 0


if __name__ == "__main__":
    sys.exit(main())
