"""The cases of tests/golden/visualize_golden.npz as plane records of tests/visualize_oracle.py, and the reference's bytes to hold them against.
Shared by the CPU test (oracle against golden) and the GPU test (kernel against oracle, and against the golden)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "visualize_golden.npz")

# kinds that may differ from the reference by one byte step on at most 1 % of their bytes (the reference's matmul / its torch.norm and the
# table's sum are not pinned operation by operation); every other case is byte-exact
BANDED = ("normal", "surface_normal", "depth_table")


def load():
    return np.load(GOLDEN)


def golden_cases(gold):
    """-> list of (name, plane, canvas, origin, key of the reference's bytes)."""
    i = {k[3:]: gold[k] for k in gold.files if k.startswith("in/")}
    rgb, acc, msk, bg = i["rgb"], i["acc"], i["msk"], i["bg"]
    canvas, origin = tuple(int(v) for v in i["canvas"]), tuple(int(v) for v in i["origin"])
    out = []

    def add(name, tag, plane, crop=False):
        out.append(("%s/%s" % (name, tag), plane, canvas if crop else None, origin if crop else (0, 0), "%s/%s" % (name, tag)))

    for name, gt, crop in (("render", i["gt"], False), ("render_u8", i["gt8"], False), ("render_crop", i["gt"], True)):
        add(name, "img", dict(kind="color", img=rgb, acc=acc), crop)
        add(name, "gt", dict(kind="gt", gt=gt, msk=msk, bg=bg), crop)
        add(name, "error", dict(kind="error", img=rgb, gt=gt, msk=msk, bg=bg, acc=acc), crop)
    add("render_opaque", "img", dict(kind="color", img=rgb, acc=acc, opaque=True))
    add("depth_linear", "img", dict(kind="depth", img=i["dpt"], curve="linear", dpt_mult=0.25, acc=acc))
    add("depth_normalize", "img", dict(kind="depth", img=i["dpt"], curve="normalize", acc=acc))
    add("depth_table", "img", dict(kind="depth", img=i["dpt"], curve="normalize", table=i["table"], dpt_mult=0.9, acc=acc))
    add("alpha", "img", dict(kind="gray", img=acc, acc=acc))
    add("alpha", "gt", dict(kind="gt", gt=msk, msk=msk, bg=bg))
    add("normal", "img", dict(kind="normal", img=i["norm"], M=i["R"], acc=acc))
    add("surface_normal", "img", dict(kind="normal", img=i["surf_norm"], M=i["R"], acc=acc))
    add("specular1", "img", dict(kind="gray", img=i["spec"], acc=acc))
    add("specular3", "img", dict(kind="color", img=i["spec3"], acc=acc))
    add("roughness", "img", dict(kind="gray", img=i["rough"], acc=acc))
    add("surface", "img", dict(kind="color", img=rgb, acc=acc))
    add("diffuse", "img", dict(kind="color", img=rgb, weight=i["spec"], weight_mode="one_minus", acc=acc))
    add("reflection", "img", dict(kind="color", img=i["env"], weight=i["spec"], weight_mode="twice", acc=acc))
    return out


def reference_rgba(gold, key):
    """The array the reference handed to cv2.imwrite, BGR(A), as (1, H, W, 4) RGBA; a 3-channel array (store_alpha_channel = False) gets alpha 255."""
    a = gold[key]
    if a.shape[-1] == 2:                        # dpt_curve = 'linear': the reference writes (depth, alpha); the depth stands on three channels here
        a = a[..., [0, 0, 0, 1]]
    rgb = a[..., [2, 1, 0]]
    alpha = a[..., 3:4] if a.shape[-1] == 4 else np.full(a.shape[:-1] + (1,), 255, np.uint8)
    return np.concatenate([rgb, alpha], -1)[None]
