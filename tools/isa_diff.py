"""Compare two device assembly files of the library kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 <SCHED_FLAGS of mfm_amd/build.py> --offload-device-only -S -o a.s mfm_amd/csrc/api.hip
    python tools/isa_diff.py a.s b.s [--out profiles/NAME.txt]

Both files are split by function symbol (`.type NAME,@function` up to its `.Lfunc_end`); comment lines and `;` comments are dropped
and the function index in local labels (`.LBB<n>_`, `.Lfunc_end<n>`, ...) and the file-wide counter of the long-branch labels
(`.Lpost_getpc<n>`) are normalised, so that a function which merely moved in the file compares equal.  Printed per function (kernels and out-of-line device functions), names demangled where c++filt is there:
`identical`, or `DIFFERS` with the resource lines of both sides (VGPRs, AGPRs, SGPRs, spills, scratch, LDS, occupancy) as the
compiler states them in the comment block after the function; functions present on one side only are listed.  Exit status 0.
"""
import argparse
import re
import shutil
import subprocess

RES = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize", "sgpr_spill_count", "vgpr_spill_count")


def functions(path):
    """{symbol: (normalised instruction lines, {resource: value})}"""
    out, name, body, res = {}, None, None, None
    pending = None                                       # the function whose trailing `; Key: value` block is being read
    with open(path, errors="replace") as f:
        for raw in f:
            line = raw.rstrip("\n")
            m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
            if m:
                name, body, res = m.group(1), [], {}
                pending = None
                continue
            if name is not None:
                if re.match(r"\.Lfunc_end\d+:", line.strip()):
                    out[name] = (body, res)
                    pending, name = name, None
                    continue
                code = line.split(";", 1)[0].strip()
                if code and not code.startswith("//"):
                    code = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc#", code)      # (long branches: one counter over the whole file)
                    body.append(re.sub(r"\.L([A-Za-z_]+)\d+_", r".L\1#_", re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1#", code)))
            elif pending is not None:
                m = re.match(r"\s*;\s*(\w+):\s*(\S+)", line)
                if m and m.group(1) in RES:
                    out[pending][1][m.group(1)] = m.group(2)
    meta_name = None                                     # spill counts: the amdhsa.kernels metadata at the end of the file
    with open(path, errors="replace") as f:
        for line in f:
            m = re.match(r"\s*\.name:\s*(\S+)", line)
            if m:
                meta_name = m.group(1)
            m = re.match(r"\s*(\.[sv]gpr_spill_count):\s*(\d+)", line)
            if m and meta_name in out:
                out[meta_name][1][m.group(1)[1:]] = m.group(2)
    return out


def demangle(names):
    if not shutil.which("c++filt") or not names:
        return {n: n for n in names}
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.split("\n")))


def short(sig):
    return re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", sig))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a"); ap.add_argument("b")
    ap.add_argument("--labels", default="parent,head")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    la, lb = a.labels.split(",")
    fa, fb = functions(a.a), functions(a.b)
    names = demangle(sorted(set(fa) | set(fb)))
    lines, same, differ = [], 0, 0
    for sym in sorted(names, key=lambda s: names[s]):
        nm = short(names[sym])
        if sym not in fa or sym not in fb:
            lines.append(f"only in {la if sym in fa else lb}: {nm}")
            continue
        if fa[sym][0] == fb[sym][0]:
            same += 1
            lines.append(f"identical  {nm}")
        else:
            differ += 1
            lines.append(f"DIFFERS    {nm}")
            for lab, (body, res) in ((la, fa[sym]), (lb, fb[sym])):
                lines.append(f"    {lab:>8}: {len(body)} lines; " + " ".join(f"{k}={res[k]}" for k in RES if k in res))
    lines.insert(0, f"{same} functions identical, {differ} differ ({la} vs {lb}; comment lines dropped, local-label function indices normalised)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
