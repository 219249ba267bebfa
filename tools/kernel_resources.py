"""What the compiler made of some kernels, without a GPU: hipcc -Rpass-analysis=kernel-resource-usage with the build's
flags on the sources named, one row per kernel whose name holds one of the substrings given.

    python tools/kernel_resources.py [--root TREE] stats.hip,picker.hip kurt_leaf_kernel find_picks_kernel

--root: another checkout of the project (the parent commit, say) instead of this one."""
import argparse
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seismic_bpmf_amd.build import ARCH, FLAGS, find_hipcc  # noqa: E402

COLUMNS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("SGPRs", "TotalSGPRs"), ("LDS B", "LDS Size"),
           ("scratch B", "ScratchSize"), ("occupancy", "Occupancy"), ("dyn. stack", "Dynamic Stack")]


def kernels(src):
    cmd = [find_hipcc(), f"--offload-arch={ARCH}"] + [f for f in FLAGS if f != "-shared"] + \
          ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise SystemExit(res.stderr[-3000:])
    rows = []
    for line in res.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            rows.append({"name": m.group(1)})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and rows:
            rows[-1][m.group(1)] = m.group(2)
    return rows


def short_name(mangled):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    name = subprocess.run([filt, mangled], capture_output=True, text=True).stdout.strip() if filt else mangled
    name = name.replace("(anonymous namespace)::", "").replace("bpmf::", "").replace("void ", "")
    return re.sub(r"\(.*", "", name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("sources", help="comma-separated files of seismic_bpmf_amd/csrc")
    ap.add_argument("names", nargs="+")
    args = ap.parse_args()
    table = []
    for src in args.sources.split(","):
        for row in kernels(os.path.join(args.root, "seismic_bpmf_amd", "csrc", src)):
            name = short_name(row["name"])
            if any(n in name for n in args.names):
                table.append((name, row))
    print(f"{'kernel':<34}" + "".join(f"{head:>11}" for head, _ in COLUMNS))
    for name, row in sorted(table, key=lambda t: t[0]):
        print(f"{name:<34}" + "".join(f"{row.get(key, '?'):>11}" for _, key in COLUMNS))


if __name__ == "__main__":
    main()
