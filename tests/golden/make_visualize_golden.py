"""Generate tests/golden/visualize_golden.npz from the reference's own visualizer (authoring container only):

    python tests/golden/make_visualize_golden.py <root of the reference tree>

The reference's code is loaded FROM THE REFERENCE TREE AT RUN TIME, the way make_fuse_golden.py loads its functions: the modules in question import
cv2, h5py and the whole engine at the top, so the definitions named in WANTED -- VolumetricVideoVisualizer.generate_type, depth_curve_fn,
normalize_depth, colormap, colormap_linear, colormap_list, normalize, save_image and the Visualization enum -- are taken out of their files through
`ast` (decorators dropped: torch.jit.script needs a source file) and executed in a namespace that holds torch, numpy, a four-line dotdict and a
cv2 stand-in whose imwrite keeps the array it is handed.  Nothing of the reference's text is written anywhere.

Per case the fixture holds the uint8 array save_image hands to cv2.imwrite -- the reference's own bytes, in BGR(A) order -- for the image and,
where the reference makes them, its ground truth and error map: "<case>/img", "<case>/gt", "<case>/error".  The inputs are stored once ("in/...");
tests/visualize_cases.py builds the planes of each case from them.  The two sampler lines generate_type's DIFFUSE and REFLECTION inputs come
from (envgs_sampler.py:413, :476) are replayed here as the torch expressions they are.  The table of the colour-map case is random, made here;
it is registered under a name of its own in the colour-map store the extracted colormap() reads, which otherwise holds 'linear': None alone.
With dpt_curve = 'linear' the reference writes TWO channels, depth and alpha (its img is the one-channel dpt_map); the fixture keeps that array as it is.  Data only."""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 27, 22
CANVAS, ORIGIN = (31, 29), (4, 3)              # (Ho, Wo), (x0, y0) of the crop case

WANTED = {"easyvolcap/utils/math_utils.py": ["normalize"],
          "easyvolcap/utils/color_utils.py": ["colormap", "colormap_linear", "colormap_list"],
          "easyvolcap/utils/depth_utils.py": ["normalize_depth", "depth_curve_fn"],
          "easyvolcap/utils/data_utils.py": ["Visualization", "save_image"],
          "easyvolcap/runners/visualizers/volumetric_video_visualizer.py": ["VolumetricVideoVisualizer.generate_type"]}


class dotdict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class FakeCv2:
    IMWRITE_JPEG_QUALITY, IMWRITE_PNG_COMPRESSION, IMWRITE_EXR_COMPRESSION, IMWRITE_EXR_COMPRESSION_PIZ = 1, 16, 49, 4

    def __init__(self):
        self.written = []

    def imwrite(self, path, img, params=None):
        self.written.append(np.array(img))
        return True


def load_reference(root):
    import enum
    import typing
    cv2 = FakeCv2()
    ns = {"torch": torch, "np": np, "os": os, "dirname": os.path.dirname, "cv2": cv2, "dotdict": dotdict, "NoneType": type(None),
          "Enum": enum.Enum, "auto": enum.auto, "Union": typing.Union, "List": typing.List,
          "cm_cpu_store": {"linear": None}, "cm_gpu_store": {}}                     # (the store's own entry for 'linear', color_utils.py:802)
    for rel, names in WANTED.items():
        tree = ast.parse(open(os.path.join(root, rel)).read())
        found = []
        for name in names:
            scope = tree.body
            for part in name.split("."):
                node = [n for n in scope if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name == part]
                if not node:
                    raise SystemExit("%s has no %s" % (rel, name))
                scope = node[0].body
            node[0].decorator_list = []
            found.append(node[0])
        exec(compile(ast.Module(body=found, type_ignores=[]), rel, "exec"), ns)
    return ns, cv2


def inputs():
    g = torch.Generator().manual_seed(910)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    inside = ((yy - 13.0) ** 2 / 150.0 + (xx - 10.0) ** 2 / 90.0) < 1.0                 # an object in front of an empty background
    acc = torch.where(inside, 0.6 + 0.4 * r(H, W), torch.zeros(H, W))
    acc[5:9, 8:12] = 1.0
    acc = acc[None, ..., None]
    rgb = r(1, H, W, 3) * 1.2 - 0.1                                                     # some values under 0 and over 1
    ties = (torch.arange(0, 22, dtype=torch.float32) * 11.0 + 0.5) / 255.0              # v * 255 lands on k + 0.5 where the product is exact
    rgb[0, 0, :, 0] = ties; rgb[0, 1, :, 1] = ties
    dpt = torch.where(inside, 2.0 + 0.05 * yy + 0.02 * xx + 0.3 * r(H, W), torch.zeros(H, W))[None, ..., None]      # zero background region
    norm = (torch.randn(1, H, W, 3, generator=g) * acc)                                 # the rasterizer's blended normal: length about acc, 0 where acc is 0
    surf = torch.randn(1, H, W, 3, generator=g)
    surf = surf / surf.norm(dim=-1, keepdim=True) * inside[None, ..., None]
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    R = (q * torch.sign(torch.det(q))).float()[None]
    msk = (r(1, H, W, 1) > 0.3).float()
    msk[0, 10:14] = r(4, W, 1)                                                          # a soft edge
    gt8 = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8)
    gt = (torch.round(r(1, H, W, 3) * 255.0) / 255.0)
    return dict(rgb=rgb, acc=acc, dpt=dpt, norm=norm, surf_norm=surf, R=R, msk=msk, gt=gt, gt8=gt8, spec=r(1, H, W, 1), spec3=r(1, H, W, 3),
                rough=r(1, H, W, 1), env=r(1, H, W, 3) * 1.1, bg=torch.tensor([0.2, 0.5, 1.0]), table=r(7, 3))


def main(root):
    torch.set_num_threads(1)
    ref, cv2 = load_reference(root)
    V = ref["Visualization"]
    inp = inputs()
    ref["cm_cpu_store"]["table"] = [row for row in inp["table"]]                       # a list: colormap() stacks it and takes colormap_list
    flat = lambda t: t.reshape(1, H * W, -1).clone()
    store = {"in/" + k: v.numpy() for k, v in inp.items()}
    store["in/canvas"], store["in/origin"] = np.array(CANVAS), np.array(ORIGIN)

    def run(case, vis_type, out_keys, batch_keys=(), crop=False, **opts):
        me = types.SimpleNamespace(store_ground_truth=True, store_image_error=True, store_alpha_channel=True, uncrop_output_images=True,
                                   dpt_curve="normalize", dpt_mult=1.0, dpt_cm="linear")
        me.__dict__.update(opts)
        output = dotdict(acc_map=flat(inp["acc"]))
        for name, key in out_keys.items():
            output[name] = key if torch.is_tensor(key) else flat(inp[key])
        batch = dotdict(meta=dotdict(H=torch.tensor([H]), W=torch.tensor([W])), R=inp["R"].clone())
        for name, key in dict(batch_keys).items():
            batch[name] = key if torch.is_tensor(key) else flat(inp[key])
        if "msk" in batch:
            output.bg_color = inp["bg"].expand(1, H * W, 3).clone()
        if crop:
            batch.meta.update(orig_h=torch.tensor([CANVAS[0]]), orig_w=torch.tensor([CANVAS[1]]), crop_x=torch.tensor([ORIGIN[0]]),
                              crop_y=torch.tensor([ORIGIN[1]]))
        imgs = ref["generate_type"](me, output, batch, V[vis_type])               # the method's own text, `me` standing for the visualizer
        for tag, im in zip(("img", "gt", "error"), imgs):
            if im is None:
                continue
            assert im.dtype == torch.float32 and im.shape[0] == 1
            del cv2.written[:]
            ref["save_image"]("x.png", im[0].numpy())
            assert len(cv2.written) == 1 and cv2.written[0].dtype == np.uint8
            store["%s/%s" % (case, tag)] = cv2.written[0]
        print("%-16s %s" % (case, " ".join("%s%s" % (t, tuple(store["%s/%s" % (case, t)].shape)) for t in ("img", "gt", "error") if "%s/%s" % (case, t) in store)))

    run("render", "RENDER", dict(rgb_map="rgb"), dict(rgb="gt", msk="msk"))
    run("render_u8", "RENDER", dict(rgb_map="rgb"), dict(rgb=flat(inp["gt8"]).float() / 255, msk="msk"))
    run("render_opaque", "RENDER", dict(rgb_map="rgb"), store_alpha_channel=False)
    run("render_crop", "RENDER", dict(rgb_map="rgb"), dict(rgb="gt", msk="msk"), crop=True)
    run("depth_linear", "DEPTH", dict(dpt_map="dpt"), dpt_curve="linear", dpt_mult=0.25)
    run("depth_normalize", "DEPTH", dict(dpt_map="dpt"))
    run("depth_table", "DEPTH", dict(dpt_map="dpt"), dpt_cm="table", dpt_mult=0.9)
    run("alpha", "ALPHA", {}, dict(msk="msk"))
    run("normal", "NORMAL", dict(norm_map="norm"))
    run("surface_normal", "SURFACE_NORMAL", dict(surf_norm_map="surf_norm"))
    run("specular1", "SPECULAR", dict(spec_map="spec"))
    run("specular3", "SPECULAR", dict(spec_map="spec3"))
    run("roughness", "ROUGHNESS", dict(rough_map="rough"))
    run("surface", "SURFACE", dict(surf_map="rgb"))
    spec = flat(inp["spec"])
    run("diffuse", "DIFFUSE", dict(dif_rgb_map=flat(inp["rgb"]).clone() * (1 - spec)))                      # envgs_sampler.py:413
    run("reflection", "REFLECTION", dict(ref_rgb_map=flat(inp["env"]) * spec * 2))                            # envgs_sampler.py:476
    path = os.path.join(HERE, "visualize_golden.npz")
    np.savez_compressed(path, **store)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
