"""Image output at the size of a test set: VIEWS views of 1200 x 1600, the eight types of configs/models/envgs.yaml per view (random maps generated on
the device: nothing is rendered and nothing is read from disk).

  device form   visualize.image_planes: one radix select for the depth range plus ONE launch that writes the eight planes as uint8 RGBA, then one
                copy of the (8, 1, H, W, 4) bytes to pinned host memory.  Reported per view: the whole call (host work included), and inside it the
                select and the plane launch on their own (device events around the two C calls), and the copy.
  torch form    what the reference's visualizer does: each type as float32 torch expressions (normalize_depth with its two topk's, normalize and
                the matmul with R for the normals, the concatenation with the alpha channel), a float32 RGBA read-back per type into pinned memory
                (kinder than the reference's pageable .to('cpu')), then save_image's NumPy quantisation on the host, timed on its own with the host clock.
  png           encode_png of one finished 1200 x 1600 RGBA plane by zlib level: host work, one thread, reported apart from everything above.

One process, both forms alternating view by view, warmed up; device events (measuring-on-mi355x: events, warm-up, median with the spread).
    python profiles/image_output_timing.py [--views 100] [--host-views 5] [--out FILE]
Needs a GPU; there is no CPU path."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != HERE]          # profiles/numbers.py must not stand in for the standard library's
sys.path.insert(0, os.path.dirname(HERE))

import argparse  # noqa: E402
import statistics  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 1200, 1600


class Span:
    """Device events around a call, read after the final synchronisation."""

    def __init__(self):
        self.pairs = []

    def __call__(self, fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a)
        e1.record()
        self.pairs.append((e0, e1))
        return out

    def times(self):
        return [a.elapsed_time(b) for a, b in self.pairs]


def line(name, t, note=""):
    return "  %-34s median %8.3f ms  min %8.3f  max %8.3f  (%d)  %s" % (name, statistics.median(t), min(t), max(t), len(t), note)


def torch_types(m):
    """The eight types as the reference builds them: float32 (P, 4) each."""
    acc = m["acc"]

    def normal(n):
        n = n / (torch.norm(n, dim=-1, keepdim=True) + 1e-8)
        n = n @ m["R"].mT
        n = n * m["flip"]
        return (n * 0.5 + 0.5) * acc

    d = m["dpt"]
    n = int(d.numel() * 0.01)
    near = d.ravel().topk(n, largest=False)[0].max()
    far = d.ravel().topk(n, largest=True)[0].min()
    dn = (1 - (d - near) / (far - near)).clip(0, 1).clip(1e-6, 1 - 1e-6)
    imgs = [m["rgb"], dn.expand(-1, 3), acc.expand(-1, 3), normal(m["norm"]), normal(m["surf"]), m["spec"].expand(-1, 3), m["base"] * (1 - m["spec"]),
            m["env"] * m["spec"] * 2]
    return [torch.cat([i, acc], -1) for i in imgs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--host-views", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_output_timing.py needs a GPU")
    from envgs_amd import _lib, visualize as vis
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    r = lambda *s: torch.rand(*s, generator=g, device=dev)
    P = H * W
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, device=dev))
    m = dict(rgb=r(P, 3), base=r(P, 3), env=r(P, 3), acc=r(P, 1), spec=r(P, 1), dpt=2 + 3 * r(P, 1), norm=r(P, 3) - 0.5, surf=r(P, 3) - 0.5, R=q,
             flip=torch.tensor([1.0, -1.0, -1.0], device=dev))
    img = lambda k: m[k].view(H, W, -1)
    acc, spec = img("acc"), img("spec")
    planes = [vis.color(img("rgb"), acc=acc), vis.depth(img("dpt"), acc=acc), vis.gray(acc, acc=acc), vis.normal(img("norm"), acc=acc),
              vis.normal(img("surf"), acc=acc, M=q), vis.gray(spec, acc=acc), vis.color(img("base"), acc=acc, weight=spec, weight_mode="one_minus"),
              vis.color(img("env"), acc=acc, weight=spec, weight_mode="twice")]
    lib = _lib.load()
    select, launch, whole, copy, tform, tcopy = Span(), Span(), Span(), Span(), Span(), Span()
    c_select, c_planes = lib.envgs_visualize_depth_range, lib.envgs_visualize_planes
    lib.envgs_visualize_depth_range = lambda *a: select(c_select, *a)                 # events around the two C calls inside image_planes
    lib.envgs_visualize_planes = lambda *a: launch(c_planes, *a)
    out = torch.empty(8, 1, H, W, 4, dtype=torch.uint8, device=dev)
    host_u8 = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)
    host_f32 = torch.empty(8, P, 4, dtype=torch.float32, pin_memory=True)

    def device_view():
        whole(vis.image_planes, planes, (H, W), None, (0, 0), out)
        copy(lambda: host_u8.copy_(out, non_blocking=True))

    def torch_view():
        imgs = tform(torch_types, m)
        tcopy(lambda: [host_f32[i].copy_(t, non_blocking=True) for i, t in enumerate(imgs)])

    for _ in range(3):
        device_view(); torch_view()
    torch.cuda.synchronize()
    for s in (select, launch, whole, copy, tform, tcopy):
        del s.pairs[:]
    wall = {"device": 0.0, "torch": 0.0}
    for _ in range(args.views):
        for name, fn in (("device", device_view), ("torch", torch_view)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[name] += time.perf_counter() - t0
    quant = []
    a = host_f32.numpy()
    for _ in range(args.host_views):
        t0 = time.perf_counter()
        b = [(a[i] * 255).clip(0, 255).round().astype(np.uint8) for i in range(8)]
        quant.append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(b[i].reshape(H, W, 4), host_u8.numpy()[i, 0]) for i in (0, 2, 5))      # RENDER, ALPHA, SPECULAR: the same rule on both sides
    mb = lambda t: t.numel() * t.element_size() / 1e6
    lines = ["image output: %d views of %d x %d, eight types per view" % (args.views, H, W),
             "device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "device form (uint8 RGBA, %.1f MB per view over the link):" % mb(host_u8),
             line("depth range (radix select)", select.times()), line("plane launch (8 planes)", launch.times(), "%.1f GB/s of the bytes written" % (
                 mb(out) / 1e3 / (statistics.median(launch.times()) * 1e-3))),
             line("image_planes, whole call", whole.times(), "select + launch + host work"), line("copy to pinned host", copy.times(), "%.1f GB/s" % (
                 mb(host_u8) / 1e3 / (statistics.median(copy.times()) * 1e-3))),
             "  wall clock per view, synchronised: %.3f ms" % (wall["device"] / args.views * 1e3),
             "torch form (float32 RGBA, %.1f MB per view over the link):" % mb(host_f32),
             line("eight types as torch expressions", tform.times()), line("copy to pinned host", tcopy.times(), "%.1f GB/s" % (
                 mb(host_f32) / 1e3 / (statistics.median(tcopy.times()) * 1e-3))),
             "  wall clock per view, synchronised: %.3f ms" % (wall["torch"] / args.views * 1e3),
             line("NumPy quantisation on the host", quant, "host clock, one thread"),
             "  RENDER, ALPHA and SPECULAR bytes equal on both sides: %s" % same,
             "ratio of the medians, device part (torch expressions + copy) : (image_planes + copy): %.1f" % (
                 (statistics.median(tform.times()) + statistics.median(tcopy.times())) / (statistics.median(whole.times()) + statistics.median(copy.times()))),
             "ratio with the host quantisation on the torch side: %.1f" % (
                 (statistics.median(tform.times()) + statistics.median(tcopy.times()) + statistics.median(quant))
                 / (statistics.median(whole.times()) + statistics.median(copy.times()))),
             "png: encode_png of one RGBA plane (%.1f MB raw), host clock, one thread:" % (H * W * 4 / 1e6)]
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = np.stack([(127 + 100 * np.sin(xx / 90.0 + k) * np.cos(yy / 70.0)).astype(np.uint8) for k in range(3)] + [np.full((H, W), 255, np.uint8)], -1)
    for name, pic in (("a smooth picture", smooth), ("the random DEPTH plane", host_u8.numpy()[1, 0])):
        for level in (0, 1, 6, 9):
            t0 = time.perf_counter()
            data = vis.encode_png(pic, level)
            lines.append("  %-24s level %d: %8.1f ms  %7.2f MB" % (name, level, (time.perf_counter() - t0) * 1e3, len(data) / 1e6))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
