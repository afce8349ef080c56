"""PTv3's index plumbing restated in plain torch integer ops, from the algorithm: space-filling-curve codes, their stable sort, the
patch padding of SerializedAttention and the pooling clusters of SerializedPooling.  Runs on the CPU and on the device; it is what
unipre3d_amd/serialization.py is compared with (and timed against), next to the recorded reference values of
tests/golden/g13_serialization.npz.

Codes: batch << 3*depth | curve(c0, c1, c2); the -trans orders swap c0 and c1.  z: bit i of c0 / c1 / c2 goes to bit 3i+2 / 3i+1 / 3i.
hilbert: Skilling's axes-to-transpose walk from the top bit down (a set bit inverts axis 0's lower bits, a clear bit exchanges the
axis' lower bits with axis 0's), the same interleave, then Gray-to-binary over the whole 3*depth bit word.
Sorts are stable: equal codes keep ascending point index.
"""
import torch

ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")


def _spread3(v):
    v = v & 0x1FFFFF
    v = (v | (v << 32)) & 0x1F00000000FFFF
    v = (v | (v << 16)) & 0x1F0000FF0000FF
    v = (v | (v << 8)) & 0x100F00F00F00F00F
    v = (v | (v << 4)) & 0x10C30C30C30C30C3
    v = (v | (v << 2)) & 0x1249249249249249
    return v


def z_code(c0, c1, c2):
    return (_spread3(c0) << 2) | (_spread3(c1) << 1) | _spread3(c2)


def hilbert_code(c0, c1, c2, depth):
    x = [c0.clone(), c1.clone(), c2.clone()]
    q = 1 << (depth - 1)
    while q > 1:
        p = q - 1
        for d in range(3):
            on = (x[d] & q) != 0
            t = (x[0] ^ x[d]) & p
            x0 = torch.where(on, x[0] ^ p, x[0] ^ t)
            if d > 0:
                x[d] = torch.where(on, x[d], x[d] ^ t)
            x[0] = x0
        q >>= 1
    g = z_code(*x)
    for s in (1, 2, 4, 8, 16, 32):
        g = g ^ (g >> s)
    return g


def encode(grid_coord, batch=None, depth=16, order="z"):
    assert order in ORDERS and 1 <= depth <= 16
    m = (1 << depth) - 1
    c = [grid_coord[:, i].long() & m for i in range(3)]
    if order.endswith("-trans"):
        c[0], c[1] = c[1], c[0]
    code = hilbert_code(*c, depth) if order.startswith("hilbert") else z_code(*c)
    if batch is not None:
        code = (batch.long() << (3 * depth)) | code
    return code


def order_inverse(code):
    order = torch.argsort(code, dim=1, stable=True)
    rows = torch.arange(code.shape[1], device=code.device).repeat(code.shape[0], 1)
    inverse = torch.zeros_like(order).scatter_(dim=1, index=order, src=rows)
    return order, inverse


def serialize(grid_coord, batch, depth, orders):
    code = torch.stack([encode(grid_coord, batch, depth, o) for o in orders])
    return (code, *order_inverse(code))


def patch_padding(offset, patch_size, device=None):
    """offset: the items' cumulative ends (host sequence or tensor).  A per-item loop, as SerializedAttention's."""
    if torch.is_tensor(offset):
        device = offset.device if device is None else device
        offset = offset.tolist()
    P, start, pstart = int(patch_size), 0, 0
    pad, unpad, cu = [], [], []
    for end in offset:
        n = end - start
        npad = n if n <= P else (n + P - 1) // P * P
        slot = torch.arange(npad, device=device)
        if npad != n:
            slot[n:] = slot[n - P:npad - P].clone()
        pad.append(slot + start)
        unpad.append(torch.arange(n, device=device) + pstart)
        cu.append(torch.arange(pstart, pstart + npad, P, dtype=torch.int32, device=device))
        start, pstart = end, pstart + npad
    cu.append(torch.tensor([pstart], dtype=torch.int32, device=device))
    return torch.cat(pad), torch.cat(unpad), torch.cat(cu)


def pool_clusters(code, pooling_depth):
    code = code >> (3 * pooling_depth)
    _, cluster, counts = torch.unique(code[0], sorted=True, return_inverse=True, return_counts=True)
    indices = torch.sort(cluster, stable=True)[1]
    idx_ptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, dim=0)])
    head_indices = indices[idx_ptr[:-1]]
    pcode = code[:, head_indices]
    return (cluster, indices, idx_ptr, head_indices, pcode, *order_inverse(pcode))
