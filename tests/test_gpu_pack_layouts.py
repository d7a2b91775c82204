"""-m gpu: every layout the batched weight pack (pack.hip) writes, byte for byte against a numpy packer.

The reference is written here from the layout formulas of include/pmf_amd.h (pmf_pack_job_t) and DESIGN.md section 3, with
the three-way bf16 split done by torch.bfloat16 conversions on the CPU (round to nearest even).  Every destination is
pre-filled with a sentinel, so a byte the kernel must leave alone (the padding the caller zeroes once) shows up when it is
written.  The written set is checked twice: against the reference (whole-buffer byte equality) and against
tests/golden/pack_written_masks.npz, the set the kernel wrote before it was vectorised -- a byte is "written" when two
launches over different sentinels agree on it.  `python tests/test_gpu_pack_layouts.py --record FILE` records that file.

A forward job and an input-gradient job of one layer never share a pack table (pmf_amd/plan.py builds the forward and the
input-gradient tables separately), so the job has no second destination and there is no sibling pairing to test.
"""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pmf_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_written_masks.npz")
PARITY = ([0, 2, 6, 8], [1, 7], [3, 5], [4])       # tap subsets of a stride-2 3x3 input gradient, one per output parity


def _ru(x, m):
    return (x + m - 1) // m * m


def job(cout, cin, khw, tr, fmt, taps=None, sub=None, woff=0):
    """one pack job: weight [cout][cin][khw]; taps = tap_idx (default all); sub = (first channel, count) packs a channel
    sub-range (w_ld = cin); woff = floats the weight starts behind a 16-byte boundary (a slice of a flat parameter buffer)"""
    return dict(cout=cout, cin=cin, khw=khw, tr=tr, fmt=fmt, taps=list(range(khw)) if taps is None else list(taps), sub=sub,
                woff=woff)


def _single_cases():
    cases = {}
    for fmt in (0, 1):
        for tr in (0, 1):
            def add(name, *a, **k):
                cases["%s-f%d-t%d" % (name, fmt, tr)] = [job(*a[:3], tr, fmt, **k)]
            add("3x3_48x36", 48, 36, 9)                        # CT 160 / 9 = 17 -> 16: last ci tile of 4, last co tile of 16
            add("3x3_20x72", 20, 72, 9, woff=1)                # ragged 20 (logits); last ci tile of 8
            add("3x3_16x5", 16, 5, 9, woff=3)                  # ct < 8, odd rows
            add("1x1_64x40", 64, 40, 1)
            add("1x1_20x5", 20, 5, 1, woff=2)
            add("1x1_32x3", 32, 3, 1, woff=1)
            add("2x2_32x72", 32, 72, 4, woff=1)                # CT 40: ci tiles 40, 32
            add("2x2_16x8", 16, 8, 4)
            add("7x7_64x3", 64, 3, 49, woff=1)                 # CT 3 = Cin
            add("7x7_32x8", 32, 8, 49)                         # CT 3: ci tiles start inside a k-octet
            add("1x3_32x40", 32, 40, 3, woff=2)                # a KHW outside {1, 4, 9, 49}
            add("3x3d12_48x40", 48, 40, 9, taps=[3, 4, 5])     # aspp.b6/b12/b18: the in-bounds taps of a dilated 3x3
            add("3x3_sub_48x80", 48, 80, 9, sub=(5, 40))       # channel sub-range of a concatenated operand, 180 bytes in
            add("1x1_sub_32x77", 32, 77, 1, sub=(3, 72), woff=1)   # odd w_ld: every row starts at another alignment
    for fmt in (0, 1):
        for p, sub in enumerate(PARITY):
            cases["3x3s2_64x36_par%d-f%d-t1" % (p, fmt)] = [job(64, 36, 9, 1, fmt, taps=sub, woff=p)]
    for cin in (3, 5, 8):
        cases["stem_64x%d-f2-t0" % cin] = [job(64, cin, 49, 0, 2, woff=cin & 3)]
    # several jobs in one launch (block_start bisection)
    cases["two_jobs"] = [job(48, 36, 9, 0, 1), job(20, 72, 9, 1, 0, woff=1)]
    cases["seven_jobs"] = [job(64, 3, 49, 0, 2, woff=3), job(48, 36, 9, 0, 1), job(48, 36, 9, 1, 1, taps=PARITY[0]),
                           job(20, 5, 1, 0, 0, woff=2), job(32, 77, 1, 1, 1, sub=(3, 72), woff=1), job(32, 72, 4, 1, 0),
                           job(64, 40, 1, 0, 1)]
    return cases


CASES = _single_cases()


def _dims(j):
    c = j["sub"][1] if j["sub"] else j["cin"]
    K, N = (j["cout"], c) if j["tr"] else (c, j["cout"])
    nt = len(j["taps"])
    if j["fmt"] == 2:
        return 1, _ru(nt * 8, 16), _ru(N, 64), 6
    return nt, _ru(K, 16 if j["fmt"] else 8), _ru(N, 64), (6 if j["fmt"] else 4)


def _nbytes(j):
    nt, k_pad, ldw, b = _dims(j)
    return nt * k_pad * ldw * b


def _weight(name, i, j):
    rng = np.random.default_rng(zlib.crc32(("%s/%d" % (name, i)).encode()))
    w = rng.uniform(-0.3, 0.3, (j["cout"], j["cin"], j["khw"])).astype(np.float32)
    flat = w.reshape(-1)
    flat[::7] = np.float32(0.15625)            # exactly a bf16 (zero residual planes)
    flat[3::11] *= np.float32(1e-3)
    flat[5::13] = 0.0
    return w


def _bf16_bits(x):
    """float32 numpy -> (bits of bf16(x) as uint16, bf16(x) back in float32), round to nearest even"""
    h = torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16)
    return h.view(torch.int16).numpy().view(np.uint16), h.float().numpy()


def ref_pack(w, j, dst):
    """the numpy packer: writes job j of weight w [cout][cin][khw] into dst (uint8, pre-filled), nothing else"""
    nt, k_pad, ldw, _ = _dims(j)
    off, cnt = j["sub"] if j["sub"] else (0, j["cin"])
    sel = w[:, off:off + cnt, :][:, :, j["taps"]]                     # [co][ci][t]
    a = sel.transpose(2, 0, 1) if j["tr"] else sel.transpose(2, 1, 0)  # [t][k][n]
    T, K, N = a.shape
    if j["fmt"] == 0:
        dst.view(np.float32).reshape(nt, k_pad, ldw)[:, :K, :N] = a
        return
    t, k, n = np.meshgrid(np.arange(T), np.arange(K), np.arange(N), indexing="ij")
    if j["fmt"] == 2:
        k, t = k + 8 * t, np.zeros_like(t)
    ks, ctl = k_pad // 16, ldw // 32
    e = (((t * ks + (k >> 4)) * ctl + (n >> 5)) * 3) * 512 + ((n & 31) + 32 * ((k & 15) >> 3)) * 8 + (k & 7)
    d16 = dst.view(np.uint16)
    x = np.ascontiguousarray(a)
    for p in range(3):
        bits, back = _bf16_bits(x)
        d16[e + 512 * p] = bits
        x = x - back
    return


def run_pack(name, sentinel):
    """launch the jobs of CASES[name] over sentinel-filled destinations; returns the destinations (uint8 numpy) and weights"""
    lib = L.lib()
    jobs_py = CASES[name]
    jobs = (L.PackJob * len(jobs_py))()
    keep, dsts, ws = [], [], []
    blocks = 0
    for i, j in enumerate(jobs_py):
        w = _weight(name, i, j)
        buf = torch.zeros(w.size + 8, dtype=torch.float32, device="cuda")     # torch allocations are 256-byte aligned
        buf[j["woff"]:j["woff"] + w.size] = torch.from_numpy(w.reshape(-1)).cuda()
        dst = torch.full((_nbytes(j),), sentinel, dtype=torch.uint8, device="cuda")
        nt, k_pad, ldw, _ = _dims(j)
        J = jobs[i]
        cin = j["cin"]
        J.w, J.dst = buf.data_ptr() + 4 * j["woff"], dst.data_ptr()
        if j["sub"]:
            J.w, J.w_ld, cin = J.w + 4 * j["sub"][0] * j["khw"], j["cin"], j["sub"][1]
        ct = lib.pmf_pack_tile_ci(cin, j["khw"])
        J.Cout, J.Cin, J.KHW, J.ntaps, J.transpose = j["cout"], cin, j["khw"], len(j["taps"]), j["tr"]
        J.K_pad, J.ldw, J.CT, J.format = k_pad, ldw, ct, j["fmt"]
        J.tiles_ci = (cin + ct - 1) // ct
        J.block_start = blocks
        for q, ti in enumerate(j["taps"]):
            J.tap_idx[q] = ti
        blocks += J.tiles_ci * ((j["cout"] + 31) // 32)
        keep.append(buf)
        dsts.append(dst)
        ws.append(w)
    tab = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).cuda()
    L.check(lib.pmf_pack_weights_batched(tab.data_ptr(), len(jobs_py), blocks,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "pmf_pack_weights_batched")
    torch.cuda.synchronize()
    return [d.cpu().numpy() for d in dsts], ws


def written_bits(name):
    """per job: packed bit mask of the bytes the kernel writes, and the destinations of the first launch"""
    a, ws = run_pack(name, 0xA5)
    b, _ = run_pack(name, 0x5A)            # every byte of the two sentinels differs: equal bytes were written
    return [np.packbits(x == y) for x, y in zip(a, b)], a, ws


@pytest.fixture(scope="module")
def golden_masks():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", sorted(CASES))
def test_pack_layout_bytes(name, golden_masks):
    masks, got, ws = written_bits(name)
    for i, j in enumerate(CASES[name]):
        ref = np.full(_nbytes(j), 0xA5, dtype=np.uint8)
        ref_pack(ws[i], j, ref)
        bad = np.flatnonzero(got[i] != ref)
        assert np.array_equal(got[i], ref), "%s job %d: %d bytes differ, first at %s" % (name, i, bad.size, bad[:8])
        assert np.array_equal(masks[i], golden_masks["%s/%d" % (name, i)]), "%s job %d: written set moved" % (name, i)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    out = {}
    for nm in sorted(CASES):
        for q, m in enumerate(written_bits(nm)[0]):
            out["%s/%d" % (nm, q)] = m
    np.savez_compressed(sys.argv[2], **out)
    print("recorded %d masks of %d cases" % (len(out), len(CASES)))
