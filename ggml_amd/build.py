"""Build driver for the native parts (no cmake needed: plain hipcc / g++ invocations).

  libcdna4_kernels.so   hand-written HIP kernels + the C-ABI of include/ggml_cdna4.h, and the GGUF reader of
                        include/ggml_cdna4_gguf.h (host code)                                 (always)
  libggml-cdna4.so      ggml backend plug-in (ggml_backend_init), compiled against the ggml headers of the
                        reference tree where they lie — only when that tree is present.  A copy is kept
                        in oracle/_ref/ beside the other binaries built from that tree, with the sha256 of
                        the plug-in and C-ABI sources it was built from; on a machine without the tree,
                        build() installs that copy if those sources are the ones in this tree.
Both land in ggml_amd/lib/ (git-ignored).
"""
import filecmp
import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "lib")
OBJ = os.path.join(ROOT, "build")
REF = os.environ.get("GGML_REFERENCE_DIR", "/root/reference")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ARCH = "gfx950"
# -ffp-contract=off: the activation quantizers must round iscale*x before the int conversion, like the CPU
HIPFLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-result"]

KERNEL_SRCS = ["quantize_act.hip", "gemv_q.hip", "mmq_i8.hip", "gemm_q_mfma.hip", "gemm_q_t64.hip", "gemm_q_sk.hip", "gemm_q_lds.hip", "convert_w.hip", "ops.hip", "exact.hip", "fattn.hip", "capi.hip", "gguf_reader.cpp", "gguf_upload.hip"]
BACKEND_SRCS = ["backend/ggml_cdna4_backend.cpp", "backend/ggml_cdna4_ops.cpp", "backend/ggml_cdna4_split.cpp"]


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed: %s\n%s\n%s" % (" ".join(cmd), r.stdout[-4000:], r.stderr[-8000:]))
    return r


def _newer(src_list, out):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(s) > t for s in src_list if os.path.exists(s))


def _headers():
    hs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    hs.append(os.path.join(ROOT, "include", "ggml_cdna4.h"))
    hs.append(os.path.join(ROOT, "include", "ggml_cdna4_gguf.h"))
    bdir = os.path.join(CSRC, "backend")
    hs += [os.path.join(bdir, f) for f in os.listdir(bdir) if f.endswith(".h")]
    return hs


def _kernel_headers():
    """headers only the kernel library's sources include (.hpp): outside the plug-in's digest, which _headers() feeds"""
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]


def build_kernels(force=False, verbose=False):
    os.makedirs(LIB, exist_ok=True)
    os.makedirs(OBJ, exist_ok=True)
    srcs = [s for s in KERNEL_SRCS if os.path.exists(os.path.join(CSRC, s))]
    objs, jobs = [], []
    for s in srcs:
        src = os.path.join(CSRC, s)
        obj = os.path.join(OBJ, s.replace("/", "_") + ".o")
        objs.append(obj)
        if force or _newer([src] + _headers() + _kernel_headers(), obj):
            jobs.append([HIPCC] + HIPFLAGS + ["-c", src, "-o", obj])
    if jobs:
        if verbose:
            print("[build] compiling %d HIP sources for %s" % (len(jobs), ARCH), file=sys.stderr)
        with ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
            list(ex.map(_run, jobs))
    out = os.path.join(LIB, "libcdna4_kernels.so")
    if jobs or not os.path.exists(out):
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", out] + objs)
    return out


def have_reference():
    return os.path.exists(os.path.join(REF, "src", "ggml-backend-impl.h"))


def _digest(paths):
    """sha256 over the repository-relative names and the contents of paths"""
    h = hashlib.sha256()
    for p in sorted(paths):
        h.update(os.path.relpath(p, ROOT).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def build_backend(force=False, verbose=False):
    """the ggml plug-in; needs the ggml headers (reference tree).  A copy goes to oracle/_ref/, with the digest of the sources it was
    built from; without the tree that copy is installed when these sources are the same.  Returns the path or None."""
    out = os.path.join(LIB, "libggml-cdna4.so")
    kept = os.path.join(ROOT, "oracle", "_ref", "libggml-cdna4.so")
    stamp = kept + ".sha256"
    srcs = [os.path.join(CSRC, s) for s in BACKEND_SRCS]
    if not all(os.path.exists(s) for s in srcs):
        return None
    if not have_reference():
        if not os.path.exists(kept):
            return out if os.path.exists(out) else None
        built_from = open(stamp).read().strip() if os.path.exists(stamp) else None
        if built_from != _digest(srcs + _headers()):
            # without the tree, ggml_amd/lib/ only ever holds an installed copy: one that does not match these sources goes too
            if os.path.exists(out):
                os.remove(out)
            print("[build] oracle/_ref/libggml-cdna4.so was built from other plug-in / C-ABI sources than these: not installed "
                  "(build() where the reference tree is makes a current one)", file=sys.stderr)
            return None
        if not (os.path.exists(out) and filecmp.cmp(kept, out, shallow=False)):
            os.makedirs(LIB, exist_ok=True)
            shutil.copy2(kept, out)
            if verbose:
                print("[build] installed the ggml backend plug-in from oracle/_ref", file=sys.stderr)
        return out
    kern = os.path.join(LIB, "libcdna4_kernels.so")
    if force or _newer(srcs + _headers() + [kern], out):
        if verbose:
            print("[build] compiling ggml backend plug-in", file=sys.stderr)
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-O2", "-std=c++17", "-fPIC", "-shared",
               "-DGGML_BACKEND_DL", "-DGGML_BACKEND_BUILD", "-DGGML_BACKEND_SHARED", "-DGGML_SHARED",
               "-I" + os.path.join(REF, "include"), "-I" + os.path.join(REF, "src"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(CSRC, "backend"),
               "-o", out] + srcs + ["-L" + LIB, "-lcdna4_kernels", "-Wl,-rpath,$ORIGIN"]
        _run(cmd)
    digest = _digest(srcs + _headers())
    if _newer([out], kept) or not os.path.exists(stamp) or open(stamp).read().strip() != digest:
        os.makedirs(os.path.dirname(kept), exist_ok=True)
        shutil.copy2(out, kept)
        with open(stamp, "w") as f:
            f.write(digest + "\n")
    return out


def build_oracle(verbose=False):
    """test infrastructure: the C restatement, and oracle/_ref when the reference tree is present"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("oracle build failed:\n" + r.stdout[-3000:] + r.stderr[-3000:])


def build_microbench(verbose=False):
    """measurement tools (tools/microbench: stand-alone probes + the -DCDNA4_ABLATIONS twin of the kernel library that
    gemm_bench_abl links).  bench.py's optional `diagnostics` legs run them when they exist; they are not part of the
    product, so a failure here is reported and ignored."""
    try:
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "microbench"), "all", "abl"], capture_output=True, text=True, timeout=1500)
        if r.returncode != 0 and verbose:
            print("[build] tools/microbench failed (ignored):\n" + r.stderr[-1500:])
        return r.returncode == 0
    except Exception as e:  # noqa: BLE001
        if verbose:
            print("[build] tools/microbench skipped:", repr(e)[:200])
        return False


def build_all(force=False, verbose=False):
    k = build_kernels(force, verbose)
    b = build_backend(force, verbose)
    build_oracle(verbose)
    build_microbench(verbose)
    return k, b


if __name__ == "__main__":
    print(build_all(force="--force" in sys.argv, verbose=True))
