"""Do two builds of the library launch the same kernels for a training step?  (Beside phase_rate.py: the same join of a rocprofv3 kernel trace with
the launch log by dispatch order.)

  SDXL_LAUNCH_LOG=<log> rocprofv3 --kernel-trace --output-format csv -d <dir> -o t -- python profiles/tools/gemm_route_trace.py step <workload> <lib.so>
      one warm-up step and one eager training step (graphs off) of a bench.py workload on the given build
  python profiles/tools/gemm_route_trace.py compare <summary.txt> <golden.json> <workload>=<dir of build A>,<dir of build B> ...
      each dir holds `log` and the trace csv of such a run.  Compares, launch by launch, (kernel name, grid, workgroup size, LDS bytes) of the whole
      trace; writes the summary, and the route table: one row per distinct GEMM problem of B's launch log (which carries the fields gemm_route reads) with
      the kernel family, configuration and split-K pass read off the kernel names A ran for it -- never from gemm_route."""
import collections, csv, json, re, sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
MAIN = ("gemm_kernel", "gemm256_kernel", "cr256_kernel", "pl_kernel", "wgrad256_kernel", "conv_wgrad3_kernel", "gemm_sk_kernel")
POST = {"splitk_reduce_kernel": "splitk_reduce", "splitk_epilogue_kernel": "splitk_epilogue"}


def step(workload, libpath):
    sys.path.insert(0, str(ROOT))
    import ctypes
    import torch
    import sdxl_amd  # noqa: F401
    import bench
    from sdxl_amd import lib, synth
    from sdxl_amd import unet as NU
    lib.LIB_PATH = Path(libpath).resolve()
    probe = ctypes.CDLL(str(lib.LIB_PATH))      # (as bench.py --lib: an older build lacks the newer entry points)
    lib.SIGNATURES = {k: v for k, v in lib.SIGNATURES.items() if hasattr(probe, k)}
    lib.TEST_HOOK_SIGNATURES = {k: v for k, v in lib.TEST_HOOK_SIGNATURES.items() if hasattr(probe, k)}
    wl = bench.WORKLOADS[workload]
    net = NU.NativeUNet(NU.make_config(), device=0)
    synth.load_synthetic(net, seed=0)
    net.set_graph_mode(False)
    net.plan(wl["B"], wl["H"], wl["W"], 77)
    b = bench.make_batch(wl, 0, torch.device("cuda", 0))
    for _ in range(2):
        net.zero_grads()
        net.forward_loss(wl["method"], b["lat"], b["noise"], b["sigma_or_t"], b["timestep"], b["ehs"], b["pooled"], b["tid"])
        net.backward(1.0, True)
        torch.cuda.synchronize()
    print(f"{workload} on {lib.LIB_PATH}: loss {net.read_loss()[0]:.6f}")
    net.close()


def read(d):
    (trace,) = sorted(Path(d).rglob("*kernel_trace.csv"))
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Dispatch_Id"]))
    g = lambda r, k: r.get(k) or r.get(k.replace("_Size", ""), "?")
    launches = [(r["Kernel_Name"], "x".join(g(r, f"Grid_Size_{a}") for a in "XYZ"), "x".join(g(r, f"Workgroup_Size_{a}") for a in "XYZ"),
                 r.get("LDS_Block_Size", r.get("LDS_Block_Size_v", "?"))) for r in rows]
    log = [l.strip().split(",") for l in open(Path(d) / "log") if l.startswith("G,")]
    return launches, log


def family(name):
    m = re.search(r"\b(\w+_kernel)\b", name)
    return m.group(1) if m else None


def route_of(name, post):
    """(kernel, cfg, fast) from a demangled kernel name: the template arguments say which instantiation ran"""
    fam = family(name)
    t = [x.strip() for x in re.search(r"<(.*)>", name).group(1).split(",")] if "<" in name else []
    num = lambda x: int(re.sub(r"[^0-9-]", "", x))
    flag = lambda x: x in ("true", "1") or x.endswith(")1")
    if fam == "gemm_kernel":      # <FORM, CONV, BN, S, BK, FAST, NW, KSP, PL>
        bn, s, bk, nw = num(t[2]), num(t[3]), num(t[4]), num(t[6])
        cfg = {(128, 2, 64, 4, False, False): 1, (128, 2, 32, 4, False, False): 2, (160, 4, 64, 8, False, False): 3, (160, 4, 64, 8, True, False): 23,
               (160, 2, 64, 4, False, False): 13, (160, 4, 64, 4, False, True): 5, (128, 4, 64, 4, False, True): 6, (160, 4, 64, 4, False, False): 43}[(bn, s, bk, nw, flag(t[7]), flag(t[8]))]
        return {"kernel": "128-row", "cfg": cfg, "fast": flag(t[5]), "post": post}
    if fam == "cr256_kernel":     # <FORM, BN, BIASG, S, PH>
        bn, deep, ph = num(t[1]), num(t[3]) == 6, len(t) > 4 and flag(t[4])
        return {"kernel": "cr256", "cfg": (33 if bn == 160 else 34) if deep else (36 if bn == 160 else 35) if ph else (31 if bn == 160 else 32), "fast": False, "post": post}
    if fam == "pl_kernel":        # <FORM, BN, PF>
        return {"kernel": "pipelined", "cfg": 8 if flag(t[2]) else 7, "fast": False, "post": post}
    return {"kernel": {"gemm256_kernel": "256x256", "wgrad256_kernel": "wgrad256", "conv_wgrad3_kernel": "conv_wgrad3", "gemm_sk_kernel": "stream-K"}[fam],
            "cfg": 0, "fast": False, "post": post}


def compare(summary, golden, pairs):
    sys.path.insert(0, str(ROOT))
    import importlib
    fields = importlib.import_module("sdxl-training-improvements_amd.lib").GEMM_DESC_FIELDS
    out, table, bad = [], {}, 0
    for pair in pairs:
        wl, dirs = pair.split("=")
        (la, ga), (lb, gb) = (read(d) for d in dirs.split(","))
        differ = [i for i, (x, y) in enumerate(zip(la, lb)) if x != y]
        same_log = len(ga) == len(gb) and all(x[:8] == y[:8] for x, y in zip(ga, gb))
        fams = collections.Counter(family(n[0]) for n in la if family(n[0]) in MAIN + tuple(POST))
        out.append(f"{wl}: {len(la)} / {len(lb)} kernel launches (two steps and the set-up), {len(differ) + abs(len(la) - len(lb))} differ in (name, grid, workgroup, LDS); "
                   f"{len(ga)} / {len(gb)} GEMM problems logged, first seven columns {'equal' if same_log else 'DIFFERENT'}")
        out.append("    " + ", ".join(f"{k} {v}" for k, v in sorted(fams.items())))
        for i in differ[:5]:
            out.append(f"    launch {i}: {la[i]} != {lb[i]}")
        bad += len(differ) + abs(len(la) - len(lb)) + (not same_log)
        # A's GEMM-family launches in dispatch order <-> the log lines: one main kernel each, then its split-K pass if it has one
        mains = [(i, n[0]) for i, n in enumerate(la) if family(n[0]) in MAIN]
        assert len(mains) == len(gb), (wl, len(mains), len(gb))
        for (i, name), rec in zip(mains, gb):
            nxt = family(la[i + 1][0]) if i + 1 < len(la) else None
            desc = tuple(int(x) for x in rec[1:1 + len(fields)])
            want = route_of(name, POST.get(nxt, "none"))
            assert table.setdefault(desc, want) == want, (wl, desc, table[desc], want)      # one problem, one route
        out.append(f"    {len(table)} distinct problems in the route table so far")
    Path(summary).write_text("\n".join(out) + "\n")
    rows = [{"problem": dict(zip(fields, d)), "route": r} for d, r in sorted(table.items())]
    Path(golden).write_text("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("\n".join(out))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(step(*sys.argv[2:4]) if sys.argv[1] == "step" else compare(sys.argv[2], sys.argv[3], sys.argv[4:]))
