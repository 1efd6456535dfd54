"""Back-to-back timing of the descriptor head behind convDa.0 at the bench shape (16 frames, 120 x 160 x 256 map, keypoints from
a real extraction of the synthetic frames):

  dense :  convDa.3 (window-resident 3x3) -> convDb + normalize -> sample_nhwc        (runs on any commit: the parent's numbers)
  sparse:  row list -> gathered 3x3 -> 1x1 + normalize on the rows -> sampling through the list

  python profiles/tools/sparse_desc_head_probe.py --mode dense|sparse|both [--kpts 2048,3072,4096] [--frames 16]

Prints one line per (mode, k): median / min of `--reps` timings of `--iters` back-to-back chains (hip events), and for the sparse
form the live fraction of the map per frame (listed pixels / map pixels) and the list length."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from pram_amd import ops, weights as W      # noqa: E402
from pram_amd.nets.sfd2 import ResNet4x     # noqa: E402


def timed(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / iters)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="both", choices=["dense", "sparse", "both"])
    ap.add_argument("--kpts", default="2048,3072,4096")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    net = ResNet4x()
    net.load_state_dict(W.make_state_dict("sfd2", net.state_dict(), seed=7), strict=True)
    net.to(dev).eval()
    img = torch.stack([W.synthetic_image(i) for i in range(a.frames)]).to(dev).contiguous()
    with torch.no_grad():
        P, _, _, _, o4 = net._backbone(img)
        da = ops.conv2d_nhwc(o4, P["convDa.w0"], P["convDa.b0"], P["convDa.s0"], P["convDa.t0"], ks=3, relu=True)
        fh, fw = da.shape[1], da.shape[2]
        for k in [int(x) for x in a.kpts.split(",")]:
            ex = net.extract_batched(img, {"min_keypoints": 128, "max_keypoints": k})
            kp, counts = ex["keypoints"], ex["counts"]
            w3, b3, w1, b1 = P["convDa.w3"], P["convDa.b3"], P["convDb.w"], P["convDb.b"]

            def dense():
                dm = ops.conv2d_nhwc(ops.conv2d_nhwc(da, w3, b3, ks=3), w1, b1, ks=1, l2norm=True)
                return ops.sample_nhwc(dm, kp, counts, 4, True)
            head = f"k={k} frames={a.frames} map={fh}x{fw} counts={counts.min().item()}..{counts.max().item()}"
            want = dense()
            if a.mode in ("dense", "both"):
                med, lo = timed(dense, a.iters, a.reps)
                print(f"dense  {head}: median {med:.1f} us  min {lo:.1f} us", flush=True)
            if a.mode in ("sparse", "both"):
                rlen = -(-min(4 * k, fh * fw) // ops.SPARSE_ROWS_TILE) * ops.SPARSE_ROWS_TILE

                def sparse():
                    return ops.sparse_descriptors(da, w3, b3, w1, b1, kp, counts, 4, rlen)
                got, _, n_rows, _ = ops.sparse_descriptors(da, w3, b3, w1, b1, kp, counts, 4, rlen, want_parts=True)
                live = (n_rows.float() / (fh * fw)).tolist()
                med, lo = timed(sparse, a.iters, a.reps)
                print(f"sparse {head}: median {med:.1f} us  min {lo:.1f} us  rlen {rlen} ({rlen / (fh * fw):.3f} of the map)  "
                      f"equal to dense {torch.equal(got, want)}  live fraction per frame min {min(live):.3f} mean {sum(live) / len(live):.3f} "
                      f"max {max(live):.3f}  [{' '.join(f'{x:.3f}' for x in live)}]", flush=True)


if __name__ == "__main__":
    main()
