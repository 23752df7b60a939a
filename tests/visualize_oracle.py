"""NumPy float32 oracle of the image output (include/envgs_visualize.h, envgs_amd/csrc/visualize.hip): the visualizer's maps as 8-bit RGBA, operation
by operation, one float32 rounding per operation, in the order the header states.  It states the semantics, the deviations from the reference
included:
  * a NaN gives the byte 0 (the reference's cast of a NaN is undefined); every clip before the byte rule keeps a NaN, as torch.clip does;
  * depth range: n = max(int(N * 0.01), 1) (the reference raises under 100 pixels), near / far the n-th smallest / largest, ranks n - 1 and N - n,
    -0 ranked with +0; far <= near gives 1 where d <= near and 0 elsewhere (the reference divides by zero); each image on its own;
  * the table colour map is the reference's FULL loop over the segments (the kernel's short-cut must give these bytes).
A plane is a dict: kind ("color", "gray", "depth", "normal", "gt", "error") and, by kind, img / weight / acc / gt / msk as (B, H, W, C) arrays
(float32; gt float32 or uint8), weight_mode (None, "one_minus", "twice"), curve ("linear", "normalize"), table (K, 3), dpt_mult, M (B, 3, 3), bg (3,),
opaque.  Missing keys are None."""
import numpy as np

F = np.float32
P_DEPTH = 0.01


def to_byte(v):
    """save_image: (img * 255).clip(0, 255).round().astype(uint8) in float32; ties to even; NaN -> 0."""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        s = np.round(np.clip(v * F(255.0), F(0.0), F(255.0)))
    return np.where(np.isnan(s), F(0.0), s).astype(np.uint8)


def depth_ranks(N, p=P_DEPTH):
    n = max(int(N * p), 1)
    return n - 1, N - n


def depth_range(depth):
    """depth: one image, any shape.  -> (near, far) float32."""
    d = np.asarray(depth, F).ravel() + F(0.0)                   # -0 + 0 = +0: ranked, and returned, as +0
    r0, r1 = depth_ranks(d.size)
    s = np.sort(d)
    return s[r0], s[r1]


def colormap_table(v, table):
    """colormap_list of the reference on v (...,) float32 in [1e-6, 1 - 1e-6]: every segment, a knot value counted by both its segments."""
    table = np.asarray(table, F)
    K = len(table)
    color = np.zeros(v.shape + (3,), F)
    for i in range(K - 1):
        b0 = i / (K - 1)
        b1 = (i + 1) / (K - 1)
        with np.errstate(invalid="ignore"):
            interp = ((v - F(b0)) / F(b1 - b0))[..., None]
            valid = (interp >= F(0.0)) & (interp <= F(1.0))
            color = color + (table[i + 1] * interp + table[i] * (F(1.0) - interp)) * valid.astype(F)
    return color


def normalize_depth(d, near, far):
    with np.errstate(invalid="ignore", divide="ignore"):
        if far <= near:
            v = np.where(d <= near, F(1.0), F(0.0)).astype(F)
        else:
            v = np.clip(F(1.0) - (d - near) / (far - near), F(0.0), F(1.0))
        return np.clip(v, F(1e-6), F(1.0 - 1e-6))


def _get(plane, key):
    v = plane.get(key)
    return None if v is None else np.asarray(v)


def _color(plane):
    img = np.asarray(plane["img"], F)
    if plane["kind"] == "gray":
        return np.repeat(img[..., :1], 3, -1)
    c = img[..., :3]
    mode = plane.get("weight_mode")
    if mode == "one_minus":
        c = c * (F(1.0) - np.asarray(plane["weight"], F)[..., :1])
    elif mode == "twice":
        c = (c * np.asarray(plane["weight"], F)[..., :1]) * F(2.0)
    else:
        assert mode is None
    return c


def _gt(plane):
    gt = np.asarray(plane["gt"])
    g = gt.astype(F) / F(255.0) if gt.dtype == np.uint8 else gt.astype(F)
    if g.shape[-1] == 1:
        g = np.repeat(g, 3, -1)
    g = g[..., :3]
    msk, bg = _get(plane, "msk"), _get(plane, "bg")
    if msk is not None and bg is not None:
        g = g + np.asarray(bg, F) * (F(1.0) - msk.astype(F)[..., :1])
    return g


def plane_values(plane):
    """-> rgb (B, H, W, 3) float32, alpha (B, H, W, 1) float32 or None (byte 255)."""
    kind = plane["kind"]
    acc, msk = _get(plane, "acc"), _get(plane, "msk")
    alpha = acc
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind in ("color", "gray"):
            c = _color(plane)
        elif kind == "depth":
            d = np.asarray(plane["img"], F)[..., 0]
            if plane.get("curve", "normalize") == "normalize":
                v = np.empty_like(d)
                for b in range(d.shape[0]):
                    near, far = depth_range(d[b])
                    v[b] = normalize_depth(d[b], near, far)
                c = colormap_table(v, plane["table"]) if plane.get("table") is not None else np.repeat(v[..., None], 3, -1)
            else:
                c = np.repeat(d[..., None], 3, -1)
            c = c * F(plane.get("dpt_mult", 1.0))
        elif kind == "normal":
            n = np.asarray(plane["img"], F)[..., :3]
            s = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]) + F(1e-8)
            u = n / s[..., None]
            M = _get(plane, "M")
            if M is not None:
                M = M.astype(F)[:, None, None]                                                   # (B, 1, 1, 3, 3)
                u = np.stack([(u[..., 0] * M[..., j, 0] + u[..., 1] * M[..., j, 1]) + u[..., 2] * M[..., j, 2] for j in range(3)], -1)
            m = u * np.array([1.0, -1.0, -1.0], F)
            c = m * F(0.5) + F(0.5)
            if acc is not None:
                c = c * acc.astype(F)[..., :1]
        elif kind == "gt":
            c = _gt(plane)
            alpha = msk
        elif kind == "error":
            d = _color(plane) - _gt(plane)
            e = np.clip((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], F(0.0), F(1.0))
            c = np.repeat(e[..., None], 3, -1)
            alpha = None if msk is None or acc is None else np.clip(msk.astype(F)[..., :1] + acc.astype(F)[..., :1], F(0.0), F(1.0))
        else:
            raise ValueError(kind)
    if plane.get("opaque"):
        alpha = None
    assert c.dtype == F
    return c, None if alpha is None else alpha.astype(F)[..., :1]


def plane_bytes(plane, canvas=None, origin=(0, 0)):
    """-> (B, Ho, Wo, 4) uint8; canvas (Ho, Wo), origin (x0, y0) of the crop; zero outside."""
    c, a = plane_values(plane)
    B, H, W = c.shape[:3]
    rgba = np.concatenate([to_byte(c), np.full((B, H, W, 1), 255, np.uint8) if a is None else to_byte(a)], -1)
    Ho, Wo = (H, W) if canvas is None else canvas
    x0, y0 = origin
    out = np.zeros((B, Ho, Wo, 4), np.uint8)
    out[:, y0:y0 + H, x0:x0 + W] = rgba
    return out


def image_planes(planes, canvas=None, origin=(0, 0)):
    return np.stack([plane_bytes(p, canvas, origin) for p in planes])
