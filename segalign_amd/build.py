"""Build libsegalign_hip.so (gfx950) in-tree with hipcc.  No GPU is needed to compile."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libsegalign_hip.so")
SOURCES = ["encode.hip", "scan.hip", "table.hip", "seeds.hip", "probe.hip", "extend.hip", "dedup.hip", "coverage.hip",
           "arena.hip", "options.hip", "profile.hip", "pool.hip", "front.hip", "core.hip", "api_setup.hip", "api_calls.hip", "api_rm.hip",
           "api_introspect.hip", "gapped.hip", "cover.hip", "api_gapped.hip", "hspchain.hip", "hsppeel.hip", "hspovl.hip", "api_hspchain.hip",
           "stitch.hip", "api_stitch.hip", "chaintrim.hip", "api_chaintrim.hip", "net.hip", "api_net.hip", "netsubset.hip",
           "api_netsubset.hip", "netclass.hip", "api_netclass.hip", "lift.hip", "api_lift.hip", "fill.hip",
           "api_fill.hip", "diff.hip", "api_diff.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]


def _newer(src, dst):
    return (not os.path.exists(dst)) or os.path.getmtime(src) > os.path.getmtime(dst)


def build_lib(force=False, verbose=False):
    hipcc = os.environ.get("HIPCC", "hipcc")
    os.makedirs(LIB_DIR, exist_ok=True)
    obj_dir = os.path.join(LIB_DIR, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    headers = [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h")]
    headers.append(os.path.join(HERE, "..", "include", "segalign_amd.h"))
    objs, procs = [], []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        op = os.path.join(obj_dir, src.replace(".hip", ".o"))
        objs.append(op)
        if force or _newer(sp, op) or any(_newer(h, op) for h in headers):
            cmd = [hipcc] + FLAGS + ["-c", sp, "-o", op]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    failed = False
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            failed = True
            sys.stderr.write("hipcc failed for %s:\n%s\n" % (src, out.decode(errors="replace")))
        elif verbose and out:
            sys.stderr.write(out.decode(errors="replace"))
    if failed:
        raise RuntimeError("hipcc build failed")
    if force or procs or not os.path.exists(LIB_PATH):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
        subprocess.check_call(cmd)
    return LIB_PATH


def kernel_resources(src="hspchain.hip"):
    """{kernel: {"vgprs", "agprs", "sgprs", "scratch", "lds", "occupancy"}} of a unit's kernels, from the compiler's own resource-usage
    remarks (device code only, nothing is written).  `python -m segalign_amd.build --resources [unit.hip]` prints them (hspchain.hip's by default)."""
    import re
    hipcc = os.environ.get("HIPCC", "hipcc")
    cmd = [hipcc] + FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", os.devnull]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode(errors="replace")
    fields = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds",
              "Occupancy [waves/SIMD]": "occupancy"}
    res, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            try:
                name = subprocess.run(["c++filt", m.group(1)], stdout=subprocess.PIPE, check=True).stdout.decode().strip()
            except (OSError, subprocess.CalledProcessError) as e:
                raise RuntimeError("kernel_resources: c++filt is needed to read the kernels' names (%s)" % e)
            name = re.sub(r"^.*::", "", re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")))
            cur = res.setdefault(name, {})
            continue
        m = re.search(r"remark: .*?\s+([A-Za-z][A-Za-z \[\]/]*): (\d+)", line)
        if m and cur is not None and m.group(1) in fields:
            cur[fields[m.group(1)]] = int(m.group(2))
    if not res:
        raise RuntimeError("kernel_resources: no resource-usage remark in the compiler's output for %s" % src)
    for name, r in res.items():
        missing = sorted(set(fields.values()) - set(r))
        if missing:
            raise RuntimeError("kernel_resources: %s: no %s in the compiler's remarks" % (name, ", ".join(missing)))
    return res


HOST_SRC = os.path.join(HERE, "host", "segalign_host.cpp")
HOST_BIN = os.path.join(HERE, "bin", "segalign_host")
RM_HOST_SRC = os.path.join(HERE, "host", "segalign_rm_host.cpp")
RM_HOST_BIN = os.path.join(HERE, "bin", "segalign_rm_host")
HOST_COMMON = os.path.join(HERE, "host", "host_common.hpp")


def build_host(force=False):
    """The C++ host harness (FASTA -> .segments) on top of the C-ABI: plain g++ + zlib, links libsegalign_hip.so."""
    build_lib()
    os.makedirs(os.path.dirname(HOST_BIN), exist_ok=True)
    hdr = os.path.join(HERE, "..", "include", "segalign_amd.h")
    for src, dst in ((HOST_SRC, HOST_BIN), (RM_HOST_SRC, RM_HOST_BIN)):
        if force or _newer(src, dst) or _newer(hdr, dst) or _newer(HOST_COMMON, dst) or _newer(LIB_PATH, dst):
            subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-Wall", "-I", os.path.join(HERE, "..", "include"), src,
                                   "-o", dst, "-L", LIB_DIR, "-lsegalign_hip", "-lz", "-Wl,-rpath," + LIB_DIR,
                                   "-Wl,-rpath,/opt/rocm/lib"])
    return HOST_BIN


if __name__ == "__main__":
    if "--resources" in sys.argv:  # --resources [unit]: hspchain.hip unless a unit such as hsppeel.hip follows
        at = sys.argv.index("--resources") + 1
        unit = sys.argv[at] if at < len(sys.argv) and sys.argv[at].endswith(".hip") else "hspchain.hip"
        for k, v in sorted(kernel_resources(unit).items()):
            print("%-32s %s" % (k, " ".join("%s=%d" % kv for kv in sorted(v.items()))))
        sys.exit(0)
    print(build_lib(force="--force" in sys.argv, verbose=True))
    print(build_host(force="--force" in sys.argv))
