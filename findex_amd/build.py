"""Builds libfmx.so (HIP kernels + C ABI) for gfx950, in-tree.

    python -m findex_amd.build [--force]

hipcc cross-compiles without a GPU; the .so lands in findex_amd/lib/ (git-ignored,
but shipped to the GPU box with the tree).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "lib")
OUT = os.path.join(OUT_DIR, "libfmx.so")
# the same library with fmx_comm.cpp's fault-injection switch compiled in (-DFMX_FAULT_INJECTION): loaded by one test only
OUT_FAULTS = os.path.join(OUT_DIR, "libfmx_faults.so")
SOURCES = ["fmx_api.cpp", "fmx_hostpar.cpp", "fmx_comm.cpp", "fmx_hostrank.cpp", "fmx_regex.cpp", "fmx_build.hip", "fmx_kernels.hip", "fmx_search.hip", "fmx_search4_onehot.hip", "fmx_search4_onehot_wide.hip", "fmx_search4_bytes.hip", "fmx_search4_onehot_kx.hip", "fmx_ktab.hip", "fmx_jump.hip", "fmx_select.hip", "fmx_locate.hip", "fmx_lcp.hip", "fmx_frontier.hip", "fmx_regex_batch.hip", "fmx_refmatch.hip", "fmx_order.hip", "fmx_sufsort.hip", "fmx_corpus.hip", "fmx_rank.hip", "fmx_passages.hip", "fmx_approx.hip", "fmx_edit.hip", "fmx_fold.hip", "fmx_classes.hip", "fmx_mstat.hip", "fmx_extract.hip", "fmx_repeats.hip", "fmx_ngrams.hip", "fmx_occ.hip", "fmx_context.hip", "fmx_merge.hip", "fmx_lines.hip", "fmx_linequery.hip"]
HEADERS = ["fmx_approx.h", "fmx_classes.h", "fmx_corpus_dev.h", "fmx_ctx_math.h", "fmx_device.h", "fmx_fold.h", "fmx_frontier.h", "fmx_host.h", "fmx_hostpar.h", "fmx_lines_dev.h", "fmx_nfa.h", "fmx_order.h", "fmx_order_math.h", "fmx_passage_math.h", "fmx_pool_deal.h", "fmx_rank_math.h", "fmx_regex.h", "fmx_search4.h"]
MAX_JOBS = 16       # hipcc processes at once
ARCH = "gfx950"


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _deps():
    return [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.join(ROOT, "include", "fmx.h")]


def _extra_flags():
    return os.environ.get("FMX_CXXFLAGS", "").split()


def _source_stamp():
    """Hash of every file a translation unit can see, and of FMX_CXXFLAGS.  The library is up to date when the stamp
    written beside it is this one -- file times say nothing on a box the tree was copied to, and a source edited WHILE a
    build runs (hipcc reads a .hip file twice, for the device and for the host) must not leave objects that disagree
    about a struct."""
    import hashlib
    h = hashlib.sha256()
    h.update(" ".join(_extra_flags()).encode())
    for d in _deps():
        h.update(os.path.basename(d).encode())
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


STAMP = OUT + ".stamp"


def _stale():
    if not os.path.exists(OUT) or not os.path.exists(STAMP) or not os.path.exists(OUT_FAULTS):
        return True
    with open(STAMP) as f:
        return f.read().strip() != _source_stamp()


def _unit_stamp(src, flags):
    """Hash of what ONE translation unit can see: its source, every header, the flags."""
    import hashlib
    h = hashlib.sha256()
    h.update(" ".join(flags).encode())
    for d in [os.path.join(CSRC, src)] + [os.path.join(CSRC, f) for f in HEADERS] + [os.path.join(ROOT, "include", "fmx.h")]:
        h.update(os.path.basename(d).encode())
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _compile(jobs, verbose):
    """Runs the hipcc commands of `jobs` [(name, obj, unit stamp, cmd)], MAX_JOBS at a time, and writes each object's stamp
    beside it."""
    from concurrent.futures import ThreadPoolExecutor

    def run(job):
        name, obj, ustamp, cmd = job
        if verbose:
            print(" ".join(cmd))
        if subprocess.call(cmd) != 0:
            raise RuntimeError("hipcc failed on " + name)
        with open(obj + ".stamp", "w") as f:
            f.write(ustamp + "\n")

    with ThreadPoolExecutor(max_workers=MAX_JOBS) as pool:
        for r in [pool.submit(run, j) for j in jobs]:
            r.result()


def build(force=False, verbose=False):
    if not force and not _stale():
        return OUT
    os.makedirs(OUT_DIR, exist_ok=True)
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=" + ARCH, "-I" + os.path.join(ROOT, "include"),
             "-I" + CSRC, "-Wall", "-Wno-unused-result"] + _extra_flags()
    # every object, and the tests' twin of fmx_comm.cpp with the fault-injection switch compiled in
    units = [(src, os.path.join(OUT_DIR, src + ".o"), flags) for src in SOURCES]
    fobj = os.path.join(OUT_DIR, "fmx_comm.cpp.faults.o")
    units.append(("fmx_comm.cpp", fobj, flags + ["-DFMX_FAULT_INJECTION"]))
    objs = [obj for _, obj, _ in units[:-1]]
    for attempt in range(3):
        stamp = _source_stamp()
        jobs = []
        for src, obj, uflags in units:
            # an object is kept when the stamp beside it names exactly what this unit would be compiled from
            ustamp = _unit_stamp(src, uflags)
            try:
                with open(obj + ".stamp") as f:
                    fresh = os.path.exists(obj) and f.read().strip() == ustamp
            except OSError:
                fresh = False
            if fresh and not force:
                continue
            jobs.append((src, obj, ustamp, [_hipcc()] + uflags + ["-x", "hip", "-c", os.path.join(CSRC, src), "-o", obj]))
        _compile(jobs, verbose)
        if _source_stamp() == stamp:
            break           # (else: the sources changed under the compilers -- again, from what they are now)
    else:
        raise RuntimeError("the sources keep changing while they are compiled")
    for out, unit_objs in ((OUT, objs), (OUT_FAULTS, [fobj if o.endswith("fmx_comm.cpp.o") else o for o in objs])):
        tmp = out + ".%d.tmp" % os.getpid()
        cmd = [_hipcc(), "-shared", "-fPIC", "--offload-arch=" + ARCH, "-o", tmp] + unit_objs + ["-ldl"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        os.replace(tmp, out)
    with open(STAMP, "w") as f:
        f.write(stamp + "\n")
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
