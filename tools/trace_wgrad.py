#!/usr/bin/env python3
"""Phase trace of one split-bf16 weight-gradient launch (conv_wgrad_s3n_k or conv_wgrad_s3_swp_k, whichever the library
selects for the case): builds a private copy of conv_wgrad.hip with -DPMF_WG_TRACE (thread 0 of every workgroup stamps
s_memtime at phase boundaries: start, loop entry, then per tile the phases listed in `per` below, loop exit, end) and
prints the median cycle count of every phase.
usage: python tools/trace_wgrad.py [case-substring] [nsplit]     (cases of tools/bench_conv.py)"""
import ctypes as C, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from pmf_amd import _lib as L
from tests import gpu_helpers as G
from tools.bench_conv import CASES, wgrad_desc

def build():
    so = "/tmp/libpmf_wg_trace.so"
    src = os.path.join(ROOT, "pmf_amd/csrc/conv_wgrad.hip")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                           "-munsafe-fp-atomics", "-DPMF_WG_TRACE"] +        # (as the Makefile: no -amdgpu-mfma-vgpr-form for this file)
                          os.environ.get("TRACE_DEFS", "").split() + [src, "-o", so])     # e.g. TRACE_DEFS="-DPMF_WG_NOMFMA"
    return C.CDLL(so)

def main(filt, ns):
    tl = L.bind(build())
    lib = L.lib()
    for name, N, H, W, ci, co, k, dil in CASES:
        if filt and filt not in name: continue
        x = torch.randn(N, H, W, ci, device="cuda"); dz = torch.randn(N, H, W, co, device="cuda")
        wd = wgrad_desc((name, N, H, W, ci, co, k, dil), x.data_ptr(), dz.data_ptr())
        wd.nsplit = ns if ns else lib.pmf_conv_wgrad_nsplit(C.byref(wd))
        part = torch.empty(lib.pmf_conv_wgrad_workspace(C.byref(wd)), dtype=torch.uint8, device="cuda")
        gw = torch.empty(co, ci, k, k, device="cuda")
        wd.partial, wd.dw_oihw = part.data_ptr(), gw.data_ptr()
        st = G.stream()
        for _ in range(300): tl.pmf_conv_wgrad(C.byref(wd), st)
        torch.cuda.synchronize()
        buf = torch.zeros(1 << 20, dtype=torch.int64, device="cuda")
        tl.pmf_wg_trace_set(C.c_void_p(buf.data_ptr()))
        tl.pmf_conv_wgrad(C.byref(wd), st)
        torch.cuda.synchronize()
        tl.pmf_wg_trace_set(C.c_void_p(0))
        t = buf.cpu().numpy().reshape(-1, 64)
        t = t[t[:, 63] > 0]
        cnt = int(np.median(t[:, 63]))
        t = t[t[:, 63] == cnt]
        d = np.diff(t[:, :cnt].astype(np.int64), axis=1)
        span = int((t[:, cnt - 1].max() - t[:, 0].min()))
        print("== %s nsplit %d: %d workgroups, %d stamps, launch span %d ticks; per-workgroup total median %d" % (
            name, wd.nsplit, len(t), cnt, span, int(np.median(t[:, cnt - 1] - t[:, 0]))))
        names = ["prologue"]
        # stamps per tile of the body that ran (the library's own selection, same PMF_WG_* environment as the traced copy)
        variant = lib.pmf_conv_wgrad_variant(C.byref(wd))
        per = {L.WG_NSPLIT: ["barrier + loads landed", "MFMAs + split(t+1) + dz prep", "fetch(t+2)"],
               L.WG_SWP: ["barrier", "dz wait + B prep", "108 MFMAs + split(t+1)", "fetch(t+2)"]}.get(variant)
        if per is None:
            print("== %s: variant %d is not a split-bf16 tiled kernel, no stamps" % (name, variant)); continue
        ntile = (cnt - 1 - 1 - 2) // len(per)
        for i in range(ntile): names += ["t%d %s" % (i, p) for p in per]
        names += ["loop exit", "reduce+write"]
        med = np.median(d, axis=0)
        for n_, m in zip(names, med): print("   %-26s %8d" % (n_, m))
        agg = {p: 0 for p in per}
        for i in range(1, ntile):
            for j, p in enumerate(per): agg[p] += med[1 + len(per) * i + j]
        print("   per tile (tiles 1..%d):" % (ntile - 1), {p: int(v / max(ntile - 1, 1)) for p, v in agg.items()})

if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "quar_256_256_3x3d2", int(sys.argv[2]) if len(sys.argv) > 2 else 0)
