"""Score-kernel tuning variants (C2 instance only, -DKGE_ONLY_ONE): the library's
own objects with kge_step.hip and kge_abi.hip recompiled under the knobs.

    python tools/variants.py build NAME -DKGE_SLOTS_PER_WAVE=128 ...   # here: KGE/_lib/libkge_var_NAME.so
    python tools/variants.py buildfull NAME -D...   # every model family (all library sources)
    python tools/variants.py run NAME [NAME ...] [-- --workload c2-50m]  # on the GPU box: bench.py per variant
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "knowledge-graph-embedding_amd", "csrc")
LIBDIR = os.path.join(ROOT, "knowledge-graph-embedding_amd", "KGE", "_lib")


# kge_step.hip under -DKGE_ONLY_ONE holds the one element-wise instance itself and calls
# none of these units; linked in, their default-knob copy of that kernel would share its name
ELEMENTWISE_UNITS = ("kge_step_transe.hip", "kge_step_distmult.hip", "kge_step_rotate.hip")


def build_lib(out, tag, recompiled, omit=()):
    """Link `out` from the objects __graft_entry__.build() made, with the units
    in `recompiled` ({source: extra flags}) compiled again as build/var/TAG_*.o
    and those in `omit` left out."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    stock = {src: os.path.join(ROOT, "build", "obj", "%s.%s.o" % (src[:-4], g._obj_key(src)))
             for src in g.SOURCES if src not in recompiled and src not in omit}
    if stock:
        g.build(force=not all(os.path.exists(o) for o in stock.values()))
    vardir = os.path.join(ROOT, "build", "var")
    os.makedirs(vardir, exist_ok=True)
    objs, procs = [], []
    for src in g.SOURCES:
        if src in omit:
            continue
        if src in stock:
            objs.append(stock[src])
            continue
        obj = os.path.join(vardir, "%s_%s.o" % (tag, src[:-4]))
        procs.append(subprocess.Popen(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] +
                                      list(recompiled[src]) + ["-c", os.path.join(CSRC, src), "-o", obj]))
        objs.append(obj)
    for p in procs:
        assert p.wait() == 0
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out], check=True)
    print("built", out)


def build(name, defines, full=False):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    if full:
        recompiled = {src: list(defines) for src in g.SOURCES}
    else:
        # the knobs are the score / update kernels' (kge_step.hip: the C2 instance only)
        # and the plan's (kge_abi.hip: KGE_STEP_WAVES, KGE_SLOTS_PER_WAVE size the launch,
        # and it refuses the families whose objects keep the default knobs)
        recompiled = {src: ["-DKGE_ONLY_ONE"] + list(defines) for src in ("kge_step.hip", "kge_abi.hip")}
    build_lib(os.path.join(LIBDIR, "libkge_var_%s.so" % name), "var_" + name, recompiled,
              omit=() if full else ELEMENTWISE_UNITS)


def run(names, extra=()):
    import json
    for n in names:
        env = dict(os.environ, KGE_LIB=os.path.join(LIBDIR, "libkge_var_%s.so" % n))
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline",
                              "--no-hbm-point"] + list(extra), env=env,
                             capture_output=True, text=True, timeout=300)
        line = [l for l in out.stdout.splitlines() if l.startswith("{")]
        if not line:
            print(n, "FAILED", out.stderr[-800:])
            continue
        d = json.loads(line[-1])
        k = (d.get("roofline") or {}).get("kernels") or {}
        ks, ku = (k.get("score_kernel") or {}).get("ms"), (k.get("update_kernel") or {}).get("ms")
        print("%-12s %.5f ms/step  KS %s  KU %s" % (n, d["ms_per_step"], ks, ku), flush=True)


if __name__ == "__main__":
    if sys.argv[1] in ("build", "buildfull"):
        build(sys.argv[2], sys.argv[3:], full=sys.argv[1] == "buildfull")
    else:   # run NAME [NAME ...] [-- bench.py arguments]
        a = sys.argv[2:]
        cut = a.index("--") if "--" in a else len(a)
        run(a[:cut], a[cut + 1:])
