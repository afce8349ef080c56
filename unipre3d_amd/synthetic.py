"""Seeded synthetic inputs of the reference's shapes -- there are no datasets
on the GPU box.  Reference-faithful regime: N(0,1) head output pushed through the reference's
activations (head.py, R1), cameras from the reference's matrix formulas (cameras.py, R0).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict

import torch

from . import cameras, head

# BASELINE.json configs: name -> sizes per GPU
CONFIGS = {
    "C1": dict(level="object", P=128, H=128, W=128, B=2, V=4),
    "C2": dict(level="object", P=128, H=256, W=256, B=32, V=4),
    "C3": dict(level="object", P=2048, H=256, W=256, B=16, V=4),
    "C4": dict(level="scene", P=40000, H=480, W=640, B=2, V=8),
    "C5": dict(level="scene", P=200000, H=480, W=640, B=1, V=8),
    # SURVEY's C4 / C5 rows read "~40 k voxels + fused pixel-Gaussians" (fusion/point_fusion.py:159-168 concatenates the voxels of the
    # unprojected pixels of the reference views, <= 8 x 480 x 640 before the 2 cm grid sampling): the same shapes with that share added
    "C4_fused": dict(level="scene", P=120000, H=480, W=640, B=2, V=8),
    "C5_fused": dict(level="scene", P=350000, H=480, W=640, B=1, V=8),
}


@dataclass
class SyntheticBatch:
    raw: torch.Tensor            # (B, 23, P) head output  (leaf for autograd)
    center: torch.Tensor         # (B, P, 3)
    world_view: torch.Tensor     # (B, V, 4, 4)
    full_proj: torch.Tensor      # (B, V, 4, 4)
    camera_center: torch.Tensor  # (B, V, 3)
    gt: torch.Tensor             # (B, V, 3, H, W)
    bg: torch.Tensor             # (3,)
    fov_deg: float
    level: str
    offset_scale: float

    def to(self, device):
        return SyntheticBatch(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in self.__dict__.items()})


def make_batch(B: int, P: int, V: int, H: int, W: int, level: str = "object", seed: int = 42,
               compact: bool = False, bg_fraction: float = 0.3) -> SyntheticBatch:
    """compact=True is the secondary 'compact-splat' regime: scale = exp(N(-4, 0.5))."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, 23, P, generator=g)
    if compact:
        raw[:, 4:7] = -4.0 + 0.5 * raw[:, 4:7]
    if level == "object":
        d = torch.randn(B, P, 3, generator=g)
        r = torch.rand(B, P, 1, generator=g) ** (1 / 3) * 0.5
        center = d / d.norm(dim=-1, keepdim=True) * r
        cams = [cameras.orbit_cameras(V, cameras.OBJECT_CAMERA_DISTANCE, cameras.OBJECT_FOV_DEG,
                                      cameras.OBJECT_ZNEAR, cameras.OBJECT_ZFAR, g) for _ in range(B)]
        fov, bgv, off = cameras.OBJECT_FOV_DEG, 0.0, 1.0
    else:
        box = torch.tensor([6.0, 5.0, 3.0])
        center = torch.rand(B, P, 3, generator=g) * box
        cams = [cameras.room_cameras(V, generator=g) for _ in range(B)]
        fov, bgv, off = cameras.SCENE_FOV_DEG, 1.0, 0.2
    wv = torch.stack([c[0] for c in cams]); fp = torch.stack([c[1] for c in cams]); cc = torch.stack([c[2] for c in cams])
    gt = torch.rand(B, V, 3, H, W, generator=g)
    is_bg = torch.rand(B, V, 1, H, W, generator=g) < bg_fraction
    gt = torch.where(is_bg, torch.full_like(gt, bgv), gt)
    return SyntheticBatch(raw=raw, center=center, world_view=wv, full_proj=fp, camera_center=cc, gt=gt,
                          bg=torch.full((3,), bgv), fov_deg=fov, level=level, offset_scale=off)


def gaussians_from_batch(batch: SyntheticBatch, max_sh_degree: int = 1) -> Dict[str, torch.Tensor]:
    """Head activations (R1).  Object level uses the reference's object branch; scene level applies the
    scene branch's per-quaternion normalisation on the same (B,23,P) layout."""
    if batch.level == "object":
        return head.process_object_output(batch.raw, batch.center, batch.offset_scale, max_sh_degree)
    B, C, P = batch.raw.shape
    flat = batch.raw.permute(0, 2, 1).reshape(B * P, C)
    idx = torch.arange(B, device=flat.device).repeat_interleave(P)[:, None]
    lists = head.process_scene_output(flat, batch.center.reshape(B * P, 3), idx, batch.offset_scale, max_sh_degree)
    return {k: torch.stack(v) for k, v in lists.items()}


def single_view_scene(P: int = 64, H: int = 48, W: int = 64, seed: int = 0, level: str = "object",
                      compact: bool = False, sh_degree: int = 1, unit_quats: bool = False):
    """Small one-view scene for unit tests: dict of float32 tensors in the operator's own layout."""
    b = make_batch(1, P, 1, H, W, level=level, seed=seed, compact=compact)
    g = gaussians_from_batch(b, 1)
    gen = torch.Generator().manual_seed(seed + 1000)
    M = (sh_degree + 1) ** 2
    shs = torch.randn(P, M, 3, generator=gen) * (0.6 if sh_degree else 1.0)
    shs[:, 0] = g["features_dc"][0, :, 0]
    rot = g["rotation"][0]
    if unit_quats:
        rot = torch.nn.functional.normalize(torch.randn(P, 4, generator=gen), dim=-1)
    import math
    t = math.tan(b.fov_deg * math.pi / 360)
    return dict(means3D=g["xyz"][0].contiguous(), opacities=g["opacity"][0].contiguous(),
                scales=g["scaling"][0].contiguous(), rotations=rot.contiguous(), shs=shs.contiguous(),
                viewmatrix=b.world_view[0, 0].contiguous(), projmatrix=b.full_proj[0, 0].contiguous(),
                campos=b.camera_center[0, 0].contiguous(), bg=b.bg.clone(), image_height=H, image_width=W,
                tanfovx=t, tanfovy=t, sh_degree=sh_degree)


def point_fusion_scene(V: int = 8, H: int = 120, W: int = 160, C: int = 32, seed: int = 0, n_init: int = 4096,
                       hole_rate: float = 0.05, focal_scale: float = 1.0):
    """Seeded scene-level fusion inputs (fusion/point_fusion.py:36-43) with realistic voxel sharing: each view's depth map is the
    nearest hit of its pixel rays on a 6 x 5 x 3 m room (floor, ceiling, four walls) and a few axis-aligned boxes, unprojected
    with computeUnprojection's formula (dataset/scannet.py:639-671: x = (u - cx) z / fx, y = (v - cy) z / fy, valid = z > 5 cm;
    ScanNet's intrinsics scaled to W, times `focal_scale`: a narrower view makes small images share voxels as full-size ones do).
    A `hole_rate` share of the pixels has no depth (invalid).  init_coord samples the valid
    points below 2.6 m, so ceiling pixels fall outside its box.
    Returns dict feat_2d_all (V,C,H,W), unprojected_coord (1,V,H,W,4), init_coord (n_init,3), c2w (V,4,4), all fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    room = torch.tensor([6.0, 5.0, 3.0])
    lo_b = torch.rand(4, 3, generator=g) * torch.tensor([4.5, 3.5, 0.0]) + torch.tensor([0.5, 0.5, 0.0])
    hi_b = lo_b + torch.rand(4, 3, generator=g) * torch.tensor([1.0, 1.0, 1.2]) + torch.tensor([0.3, 0.3, 0.3])
    fx = fy = 577.87 * W / 640.0 * focal_scale
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    u = torch.arange(W, dtype=torch.float32).view(1, -1).expand(H, W)
    v = torch.arange(H, dtype=torch.float32).view(-1, 1).expand(H, W)
    dirs_cam = torch.stack([(u - cx) / fx, (v - cy) / fy, torch.ones(H, W)], -1).reshape(-1, 3)   # unit depth per ray
    out, c2ws = [], []
    for _ in range(V):
        eye = torch.rand(3, generator=g) * torch.tensor([3.0, 2.5, 0.6]) + torch.tensor([1.5, 1.25, 1.2])
        yaw = float(torch.rand(1, generator=g)) * 2 * math.pi
        pitch = -0.2 - 0.3 * float(torch.rand(1, generator=g))
        fwd = torch.tensor([math.cos(yaw) * math.cos(pitch), math.sin(yaw) * math.cos(pitch), math.sin(pitch)])
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]))
        right = right / right.norm()
        down = torch.linalg.cross(fwd, right)
        R = torch.stack([right, down, fwd], 1)                       # camera x right, y down, z forward
        c2w = torch.eye(4)
        c2w[:3, :3], c2w[:3, 3] = R, eye
        d = dirs_cam @ R.T                                           # world direction per unit camera depth
        # depth of the nearest surface: the room's planes from inside, then the boxes (slab test)
        with torch.no_grad():
            inv = 1.0 / torch.where(d.abs() < 1e-9, torch.full_like(d, 1e-9), d)
            t_room = torch.where(d > 0, (room - eye) * inv, (0 - eye) * inv).min(1).values
            t = t_room
            for b in range(lo_b.shape[0]):
                t0, t1 = (lo_b[b] - eye) * inv, (hi_b[b] - eye) * inv
                tn, tf = torch.minimum(t0, t1).max(1).values, torch.maximum(t0, t1).min(1).values
                hit = (tn <= tf) & (tn > 0)
                t = torch.where(hit & (tn < t), tn, t)
        depth = t.reshape(H, W)
        depth = torch.where(torch.rand(H, W, generator=g) < hole_rate, torch.zeros_like(depth), depth)
        z = depth
        x = (u - cx) * z / fx
        y = (v - cy) * z / fy
        cam = torch.stack([x, y, z, torch.ones_like(z)], -1).reshape(-1, 4).T
        world = (c2w @ cam)[:3]
        valid = (cam[2] > 5e-2).float()
        out.append(torch.cat([world, valid.unsqueeze(0)], 0).T.reshape(H, W, 4))
        c2ws.append(c2w)
    uc = torch.stack(out).unsqueeze(0).contiguous()
    pts = uc.reshape(-1, 4)
    pts = pts[(pts[:, 3] != 0) & (pts[:, 2] < 2.6)][:, :3]
    init = pts[torch.randint(0, pts.shape[0], (n_init,), generator=g)].contiguous()
    feat = torch.randn(V, C, H, W, generator=g)
    return {"feat_2d_all": feat, "unprojected_coord": uc, "init_coord": init, "c2w": torch.stack(c2ws)}


def sparse_voxel_scene(batch: int = 2, voxel: float = 0.036, seed: int = 0, channels: int = 6):
    """Seeded surface-like sparse voxel input for the scene backbones (occupancy of real scans, not uniform noise): per batch item
    the floor, ceiling and four walls of a 6 x 5 x 3 m room, a few axis-aligned boxes and two spheres, sampled at half the voxel
    size and voxelized.  Rows are in ascending (batch, d0, d1, d2) order.  Returns dict indices (N,4) int32 (batch, d0, d1, d2),
    spatial_shape [D0, D1, D2], batch_size, features (N, channels) N(0,1), all on the CPU (about 115 k voxels per item at 3.6 cm)."""
    g = torch.Generator().manual_seed(seed)
    room = torch.tensor([6.0, 5.0, 3.0])
    h = voxel / 2

    def plane(a, b, axis, at, lo=(0.0, 0.0)):   # points of the plane axis = at over [lo, lo + (a, b)] in the other two axes
        u = torch.arange(0.0, a, h) + lo[0]
        v = torch.arange(0.0, b, h) + lo[1]
        uu, vv = torch.meshgrid(u, v, indexing="ij")
        cols = [uu.reshape(-1), vv.reshape(-1)]
        cols.insert(axis, torch.full_like(cols[0], at))
        return torch.stack(cols, 1)

    items = []
    for bi in range(batch):
        pts = [plane(6.0, 5.0, 2, 0.0), plane(6.0, 5.0, 2, 2.98), plane(5.0, 3.0, 0, 0.0), plane(5.0, 3.0, 0, 5.98),
               plane(6.0, 3.0, 1, 0.0), plane(6.0, 3.0, 1, 4.98)]
        for _ in range(3):
            lo = torch.rand(3, generator=g) * torch.tensor([4.0, 3.0, 0.0]) + 0.5
            sz = torch.rand(3, generator=g) * torch.tensor([1.0, 1.0, 1.0]) + 0.4
            for ax in range(3):
                o = [a for a in range(3) if a != ax]
                for at in (lo[ax], lo[ax] + sz[ax]):
                    p = plane(float(sz[o[0]]), float(sz[o[1]]), ax, float(at), (float(lo[o[0]]), float(lo[o[1]])))
                    pts.append(p)
        for _ in range(2):
            c = torch.rand(3, generator=g) * torch.tensor([4.0, 3.0, 1.0]) + torch.tensor([1.0, 1.0, 1.0])
            r = 0.3 + 0.4 * float(torch.rand(1, generator=g))
            n = int(4 * math.pi * r * r / (h * h))
            d = torch.randn(n, 3, generator=g)
            pts.append(c + r * d / d.norm(dim=1, keepdim=True))
        p = torch.cat(pts)
        p = p + (torch.rand(p.shape, generator=g) - 0.5) * (0.2 * voxel)
        p = torch.minimum(torch.maximum(p, torch.zeros(3)), room - 1e-4)
        q = torch.floor(p / voxel).long()
        items.append(torch.cat([torch.full((q.shape[0], 1), bi, dtype=torch.long), q], 1))
    shape = [int(math.ceil(float(x) / voxel)) for x in room]
    idx = torch.unique(torch.cat(items), dim=0)   # sorted rows: ascending (batch, d0, d1, d2)
    return {"indices": idx.to(torch.int32).contiguous(), "spatial_shape": shape, "batch_size": batch,
            "features": torch.randn(idx.shape[0], channels, generator=g)}
