"""The four contractions of include/unipre3d_sparseconv.h (u3d_spconv_gemm, _wgrad, _colsum, _dupsum) stated exactly as the header does,
with torch index operations in int64 / fp64, and builders of the hand-made tables that tests/test_gpu_sparseconv_kernels.py runs them on.

Every builder returns its table together with the facts it claims (which rows are live, which (block, tap) or (step, tap) cells hold no
source); `block_tap_live` reads the same facts back from any table with a plain loop, and the CPU tests compare the two."""
import os
import re

import numpy as np
import torch


def header_macros():
    """the class boundaries of include/unipre3d_sparseconv.h: {"SMALL_C": 8, "TILE": 64, "KSTEP": 32, "WAVE_SUM_SPLITS": 64}"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "unipre3d_sparseconv.h")).read()
    return {name: int(re.search(rf"#define U3D_SPCONV_{name} (\d+)", text).group(1)) for name in ("SMALL_C", "TILE", "KSTEP", "WAVE_SUM_SPLITS")}


# ---- references --------------------------------------------------------------------------------------------------------------------------------
def _i64(t):
    return None if t is None else torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).long().cpu()


def _f64(t):
    return None if t is None else torch.as_tensor(t).double().cpu()


def gemm_ref(A, W, bias, table, list_row=None, mask=None, out_rows=None):
    """u3d_spconv_gemm.  A (Ra, Cin), W (K, Cin, Cout), bias (Cout) or None.
    table mode (list_row None): table (R, K), Y[o] = bias + sum_k A[table[o, k]] W[k] over the entries >= 0.
    list mode: table is list_src (R), Y[list_row[e]] = bias + A[list_src[e] // K] W[list_src[e] % K] (entries < 0: the bias alone).
    mask: rows with mask[o] != o are 0.  Returns fp64 (out_rows or R, Cout); rows no entry writes stay 0."""
    A, W, bias, table, list_row, mask = _f64(A), _f64(W), _f64(bias), _i64(table), _i64(list_row), _i64(mask)
    K, Cout = W.shape[0], W.shape[2]
    R = table.shape[0]
    Y = torch.zeros(R if out_rows is None else out_rows, Cout, dtype=torch.float64)
    if list_row is None:
        out = torch.arange(R)
        for k in range(K):
            rows = torch.nonzero(table[:, k] >= 0).flatten()
            if rows.numel():
                Y.index_add_(0, rows, A[table[rows, k]] @ W[k])
    else:
        out = list_row
        for k in range(K):
            e = torch.nonzero((table >= 0) & (table % K == k)).flatten()
            if e.numel():
                Y.index_add_(0, list_row[e], A[table[e] // K] @ W[k])
    if bias is not None:
        Y.index_add_(0, out, bias.expand(out.numel(), Cout))
    if mask is not None:
        Y[out[mask[out] != out]] = 0
    return Y


def wgrad_ref(A, G, table, gather_g):
    """u3d_spconv_wgrad: dW[k] = sum over rows o with table[o, k] >= 0 of A[ia]^T G[ig]; (ia, ig) = (table[o, k], o) (gather_g == 0) or
    (o, table[o, k]) (gather_g == 1).  fp64 (K, Cin, Cout)."""
    A, G, table = _f64(A), _f64(G), _i64(table)
    K = table.shape[1]
    dW = torch.zeros(K, A.shape[1], G.shape[1], dtype=torch.float64)
    for k in range(K):
        rows = torch.nonzero(table[:, k] >= 0).flatten()
        if rows.numel():
            src = table[rows, k]
            dW[k] = A[rows].t() @ G[src] if gather_g else A[src].t() @ G[rows]
    return dW


def colsum_ref(G):
    """u3d_spconv_colsum: db[c] = sum_o G[o, c], fp64."""
    return _f64(G).sum(0)


def dupsum_ref(X, first, nxt):
    """u3d_spconv_dupsum: out[r] = X[r] + X[next[r]] + X[next[next[r]]] + ... where first[r] == r, else 0; fp64."""
    X, first, nxt = _f64(X), _i64(first), _i64(nxt)
    out = torch.zeros_like(X)
    heads = torch.nonzero(first == torch.arange(len(first))).flatten()
    cur = heads.clone()
    while heads.numel():
        out[heads] += X[cur]
        cur = nxt[cur]
        keep = cur >= 0
        heads, cur = heads[keep], cur[keep]
    return out


# ---- facts read back from a table ----------------------------------------------------------------------------------------------------------
def block_tap_live(table, rows_per_block):
    """(blocks, K) bool by a plain loop: does any row of the block hold a source at the tap?  (rows_per_block = TILE: the GEMM's tap
    skipping; = KSTEP: the weight gradient's step skipping)"""
    table = np.asarray(table)
    R, K = table.shape
    nb = -(-R // rows_per_block)
    live = np.zeros((nb, K), dtype=bool)
    for o in range(R):
        for k in range(K):
            if table[o, k] >= 0:
                live[o // rows_per_block, k] = True
    return live


def live_rows(table):
    table = np.asarray(table)
    return [o for o in range(table.shape[0]) if (table[o] >= 0).any()]


def _blocks(R, per):
    return -(-R // per)


def _claim(rows, cells):
    return {"live_rows": sorted(int(r) for r in rows), "cells": np.asarray(cells, dtype=bool)}


# ---- table builders: (table (R, K) int32, claims) ---------------------------------------------------------------------------------------------
# `per` is the block length the claims are stated for (TILE for the GEMM, KSTEP for the weight gradient); sources are rows of a
# tensor with `n_src` rows, which may be more or fewer than R.
GEMM_PATTERNS = ("dense", "sparse", "centre_tap", "empty", "block_last_row", "block_tap", "one_source")
WGRAD_PATTERNS = ("dense", "sparse", "step_last_row", "empty_steps", "empty_tap", "last_row_only")


def build_table(pattern, R, K, n_src, per, seed=0):
    """dense            every entry a random source
    sparse           about 15 % of the entries
    centre_tap       tap K // 2 only
    empty            all -1
    block_last_row   only the last row of every block of `per` rows (of a partial last block: row R - 1), every tap
    block_tap        block j holds sources at tap j % K only
    one_source       every entry points at the same row of the source tensor
    step_last_row    only rows o with o % per == per - 1, every tap
    empty_steps      blocks j with j % 3 != 0 hold nothing (j % 3 == 0: dense)
    empty_tap        tap K // 2 is -1 everywhere, the others dense
    last_row_only    row R - 1 alone, every tap"""
    g = np.random.default_rng(seed)
    src = g.integers(0, n_src, size=(R, K)).astype(np.int32)
    T = np.full((R, K), -1, dtype=np.int32)
    nb = _blocks(R, per)
    rows = np.arange(R)
    blk = rows // per
    every_row, all_cells, no_cells = list(range(R)), np.ones((nb, K), bool), np.zeros((nb, K), bool)
    if pattern == "dense":
        return src, _claim(every_row, all_cells)
    if pattern == "sparse":
        keep = g.random((R, K)) < 0.15
        T[keep] = src[keep]
        cells = no_cells.copy()
        o, k = np.nonzero(keep)
        cells[o // per, k] = True
        return T, _claim(np.nonzero(keep.any(1))[0], cells)
    if pattern == "centre_tap":
        T[:, K // 2] = src[:, K // 2]
        cells = no_cells.copy()
        cells[:, K // 2] = True
        return T, _claim(every_row, cells)
    if pattern == "empty":
        return T, _claim([], no_cells)
    if pattern == "block_last_row":
        last = [min((j + 1) * per, R) - 1 for j in range(nb)]
        T[last] = src[last]
        return T, _claim(last, all_cells)
    if pattern == "block_tap":
        T[rows, blk % K] = src[rows, blk % K]
        cells = no_cells.copy()
        cells[np.arange(nb), np.arange(nb) % K] = True
        return T, _claim(every_row, cells)
    if pattern == "one_source":
        T[:] = int(g.integers(0, n_src))
        return T, _claim(every_row, all_cells)
    if pattern == "step_last_row":
        last = rows[rows % per == per - 1]
        T[last] = src[last]
        cells = no_cells.copy()
        cells[: R // per] = True
        return T, _claim(last, cells)
    if pattern == "empty_steps":
        keep = blk % 3 == 0
        T[keep] = src[keep]
        cells = no_cells.copy()
        cells[0::3] = True
        return T, _claim(rows[keep], cells)
    if pattern == "empty_tap":
        T[:] = src
        T[:, K // 2] = -1
        cells = all_cells.copy()
        cells[:, K // 2] = False
        return T, _claim(every_row if K > 1 else [], cells)
    if pattern == "last_row_only":
        T[R - 1] = src[R - 1]
        cells = no_cells.copy()
        cells[nb - 1] = True
        return T, _claim([R - 1], cells)
    raise ValueError(pattern)


LIST_PATTERNS = ("tap_major", "shuffled", "empty", "one_tap")


def build_list(pattern, R, K, n_src, seed=0):
    """(list_row (R) a permutation of the outputs, list_src (R) = source * K + tap or -1, claims): entries in tap-major order (about a
    tenth dropped), the same shuffled, all dropped, or every entry at tap K - 1.  claims: the outputs that have a source, and the taps used."""
    g = np.random.default_rng(seed)
    list_row = g.permutation(R).astype(np.int32)
    tap = g.integers(0, K, size=R)
    source = g.integers(0, n_src, size=R)
    dropped = g.random(R) < 0.1
    if pattern == "empty":
        dropped[:] = True
    if pattern == "one_tap":
        tap[:] = K - 1
    if pattern in ("tap_major", "one_tap"):
        order = np.argsort(np.where(dropped, K, tap), kind="stable")     # dropped entries last, as u3d_spconv_down_emit orders them
        tap, source, dropped = tap[order], source[order], dropped[order]
    list_src = np.where(dropped, -1, source * K + tap).astype(np.int32)
    return list_row, list_src, {"live_outputs": sorted(int(o) for o in list_row[~dropped]), "taps": sorted({int(t) for t in tap[~dropped]})}


def build_mask(R, seed=0):
    """(R) int32: mask[o] == o for row 0 and about 60 % of the rows, a LOWER row elsewhere (SubM's `first`); the kept rows"""
    g = np.random.default_rng(seed)
    o = np.arange(R)
    keep = (g.random(R) < 0.6) | (o == 0)
    lower = (g.random(R) * o).astype(np.int64)           # < o for o > 0
    mask = np.where(keep, o, lower).astype(np.int32)
    return mask, [int(r) for r in o[keep]]


def build_chains(N, lengths, order="ascending", seed=0):
    """(first, next) int32 over N rows: chains of the given lengths on randomly chosen rows (the rest stand alone), each chain's rows
    visited in ascending row order (as the maps emit them) or descending.  Rows that are not their chain's head have first[r] != r.
    Also returns the chains as row lists in visiting order."""
    g = np.random.default_rng(seed)
    assert sum(lengths) <= N
    rows = g.permutation(N)
    first, nxt = np.arange(N, dtype=np.int32), np.full(N, -1, dtype=np.int32)
    chains, at = [], 0
    for l in lengths:
        c = np.sort(rows[at:at + l])
        at += l
        if order == "descending":
            c = c[::-1]
        first[c] = c[0]
        nxt[c[:-1]] = c[1:]
        chains.append([int(r) for r in c])
    chains += [[int(r)] for r in rows[at:]]
    return first, nxt, chains
