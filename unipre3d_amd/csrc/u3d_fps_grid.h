// Furthest point sampling of ONE cloud over SEVERAL workgroups (internal to u3d_pointops.hip, included inside its anonymous namespace
// after dist2 / sum3_pk / wave_max_u32 / fps_tie_key / fps_decode, which it reuses; in the manner of u3d_knn_core.h).  DESIGN.md,
// "Furthest point sampling over a grid of workgroups", carries the protocol's argument; this comment is its short form.
//
//  * A segment (a cloud of the dense form, or the rows [offset[s-1], offset[s]) of the offset-batched form) is cut into slices of
//    FG_P = 4096 rows, one 1024-thread workgroup per slice, 4 rows per lane: coordinates and running minimum distances stay in
//    registers for the whole call -- nothing is re-read per selection, no scratch, no distance array in memory.
//  * The local half of a selection is fps_kernel's: v_min_u32 / v_max_u32 on the distance bit patterns, the tie key only for the
//    rows at the wave maximum, one ds_max_u64 per wave on a triple-buffered LDS word, one barrier.
//  * A segment of ONE slice stops there.  A segment of G > 1 slices meets once per selection: lane 0 of every workgroup posts its
//    (distance bits << 32 | inverted tie key) with one agent-scope 64-bit atomic max on slot[j mod 3] of the segment, waits for that
//    atomic's acknowledgement (s_waitcnt vmcnt(0)), adds 1 to the segment's arrival counter, polls the counter until it shows G * j
//    (the counter only grows: no reset, no ABA), reads the slot back and hands it to its workgroup through LDS.  Every shared word
//    is written ONLY by agent-scope read-modify-write atomics and read ONLY by agent-scope atomic loads (they bypass the CU's L1;
//    the form "8-byte agent atomics on both sides": no line is ever dirty in an L2, so there is nothing for a release fence to
//    write back or for an acquire fence to invalidate -- what orders post before arrival is the wait between them).  The winner's
//    coordinates are read from the INPUT, which nobody writes.
//  * Slot recycling: slice 0 clears slot[(j + 1) mod 3] just before it arrives at meeting j.  It has passed the wait of meeting
//    j - 1 by then, so every workgroup has arrived at j - 1, hence finished reading the slot of meeting j - 2 = (j + 1) mod 3.
//    Nobody posts to that slot before passing the wait of meeting j, which needs slice 0's arrival at j, which slice 0 issues only
//    after the clear was acknowledged.  The slot of meeting j - 1 may still be being read: that is why two slots are not enough.
//  * Workgroup -> (segment, slice) on the device: every workgroup walks the b offsets (wave-uniform scalar loads).
//  * Every wait is bounded by FG_WAIT_TICKS of the constant 100 MHz clock; on give-up the status word is set, the workgroup fills the
//    rest of its segment's outputs with -1 and returns; the others follow when their own waits see the status word.
#pragma once

constexpr int FG_THREADS = 1024, FG_PPT = 4, FG_P = FG_THREADS * FG_PPT, FG_MAX_WG = 256;
constexpr unsigned long long FG_WAIT_TICKS = 200000000ull;   // 2 s of the 100 MHz constant clock: a legitimate wait is microseconds
constexpr size_t FG_WS_LINE = 128;                           // workspace: line 0 = status word, line 1 + s = segment s (slots at +0, counter at +64)
constexpr uint32_t FG_STATUS_TIMEOUT = 1u, FG_STATUS_GRID = 2u;

typedef __attribute__((address_space(1))) unsigned long long fg_gu64;
typedef __attribute__((address_space(1))) uint32_t fg_gu32;
#define FG_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

inline size_t fg_workspace_bytes(int b) { return FG_WS_LINE * ((size_t)(b > 0 ? b : 0) + 1); }

// lane 0 only.  false: gave up (budget spent, or another workgroup set the status word)
__device__ __forceinline__ bool fg_wait(fg_gu64* cnt, unsigned long long target, fg_gu32* status) {
  if (__hip_atomic_load(cnt, FG_RLX_AGENT) >= target) return true;
  const unsigned long long t0 = wall_clock64();
  for (uint32_t spin = 1u;; ++spin) {
    __builtin_amdgcn_s_sleep(1);
    if (__hip_atomic_load(cnt, FG_RLX_AGENT) >= target) return true;
    if ((spin & 15u) == 0u) {
      if (__hip_atomic_load(status, FG_RLX_AGENT) != 0u) return false;
      if (wall_clock64() - t0 > FG_WAIT_TICKS) {
        __hip_atomic_fetch_or(status, FG_STATUS_TIMEOUT, FG_RLX_AGENT);
        return false;
      }
    }
  }
}

// dense != 0: b clouds of n rows, m selections each, indices relative to the cloud, lg = log2 opt_n_threads(n) from the host (evaluated
// in double as u3d_furthest_point_sampling does); offset / new_offset unused.  dense == 0: n rows and m outputs in all, segments from the
// clamped offsets, absolute rows, lg from the largest segment (integer floor(log2), capped at 10).
template <int CM>
__global__ __launch_bounds__(FG_THREADS) void fps_grid_kernel(int b, int n, int m, int dense, int lg_dense, const float* __restrict__ xyz,
                                                              const int32_t* __restrict__ offset, const int32_t* __restrict__ new_offset,
                                                              unsigned char* __restrict__ ws, int32_t* __restrict__ idx) {
  __shared__ unsigned long long s_best[3];
  __shared__ unsigned long long s_win;
  __shared__ int s_ok;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t wave_base = (uint32_t)__builtin_amdgcn_readfirstlane(tid & ~63);
  fg_gu32* status = (fg_gu32*)ws;

  // which segment and slice this workgroup serves
  int seg = -1, slice = 0, G = 0, len = 0, mreq = 0, nmax = 0;
  long long start = 0, mstart = 0, acc = 0;
  {
    int prev = 0, nprev = 0;
    for (int s = 0; s < b; ++s) {
      long long st, mst;
      int ln, mr;
      if (dense) {
        st = (long long)s * n; mst = (long long)s * m; ln = n; mr = m;
      } else {
        const int en = min(max(offset[s], 0), n), men = min(max(new_offset[s], 0), m);
        st = prev; mst = nprev;
        ln = en > prev ? en - prev : 0; mr = men > nprev ? men - nprev : 0;
        prev = en; nprev = men;
      }
      nmax = max(nmax, ln);
      const int g = mr == 0 ? 0 : (ln == 0 ? 1 : (ln + FG_P - 1) / FG_P);   // a segment without a request needs nobody
      if (seg < 0 && (long long)blockIdx.x < acc + g) {
        seg = s; slice = (int)((long long)blockIdx.x - acc); G = g; len = ln; mreq = mr; start = st; mstart = mst;
      }
      acc += g;
    }
  }
  if (acc > (long long)gridDim.x) {   // offsets that go back and forth can ask for more slices than rows: every workgroup sees the same sum
    if (blockIdx.x == 0) {
      if (tid == 0) __hip_atomic_fetch_or(status, FG_STATUS_GRID, FG_RLX_AGENT);
      const long long total = dense ? (long long)b * m : (long long)m;
      for (long long q = tid; q < total; q += FG_THREADS) idx[q] = -1;
    }
    return;
  }
  if (seg < 0) return;
  int32_t* out = idx + mstart;
  if (len == 0) {                     // an empty segment that is asked for selections
    for (int q = tid; q < mreq; q += FG_THREADS) out[q] = -1;
    return;
  }
  const int lg = dense ? lg_dense : min(10, 31 - __clz(nmax));
  const uint32_t bs = 1u << lg;
  const float* pts = xyz + start * 3;
  const int32_t rel = dense ? 0 : (int32_t)start;               // ragged indices are absolute rows
  fg_gu64* slots = (fg_gu64*)(ws + FG_WS_LINE * ((size_t)seg + 1));
  fg_gu64* cnt = (fg_gu64*)(ws + FG_WS_LINE * ((size_t)seg + 1) + 64);

  if (tid < 3) s_best[tid] = 0ull;
  const uint32_t k0 = (uint32_t)slice * FG_P + (uint32_t)tid;   // this lane's rows of the segment: k0 + i * FG_THREADS
  float x[FG_PPT], y[FG_PPT], z[FG_PPT];
  uint32_t t[FG_PPT];                                            // running minimum squared distance, as its bit pattern
  uint32_t have = 0u;                                            // bit i: slot i holds a row of the segment
#pragma unroll
  for (int i = 0; i < FG_PPT; ++i) {
    const uint32_t k = k0 + (uint32_t)(i * FG_THREADS);
    const bool v = k < (uint32_t)len;
    have |= v ? 1u << i : 0u;
    x[i] = v ? pts[(size_t)k * 3] : 0.f; y[i] = v ? pts[(size_t)k * 3 + 1] : 0.f; z[i] = v ? pts[(size_t)k * 3 + 2] : 0.f;
    t[i] = v ? __float_as_uint(1e10f) : 0u;                     // padding slots: distance 0, and never a candidate below
  }
  __syncthreads();
  int old = 0, cur = 1, nxt = 2;
  if (slice == 0 && tid == 0) out[0] = rel;
  for (int j = 1; j < mreq; ++j) {
    const float* c = pts + (size_t)old * 3;
    const float ox = c[0], oy = c[1], oz = c[2];
    uint32_t lmax = 0u;
#pragma unroll
    for (int i = 0; i < FG_PPT; i += 2) {
#pragma clang fp contract(off)
      const f32x2 dx = f32x2{x[i], x[i + 1]} - ox, dy = f32x2{y[i], y[i + 1]} - oy, dz = f32x2{z[i], z[i + 1]} - oz;
      const f32x2 d = sum3_pk<CM>(dx, dy, dz);
      t[i] = min(t[i], __float_as_uint(d.x));
      t[i + 1] = min(t[i + 1], __float_as_uint(d.y));
      lmax = max(lmax, max(t[i], t[i + 1]));
    }
    const uint32_t wmax = wave_max_u32(lmax);
    uint32_t btk = 0u;                               // largest inverted tie key among this wave's rows at distance wmax
#pragma unroll
    for (int i = 0; i < FG_PPT; ++i) {
      // (padding slots are masked out of the ballot, not skipped in the walk: a wave of the last slice that holds no row at all has wmax = 0 in
      //  every slot of every lane, and walking those 256 bits on the scalar unit cost 6.7 us per selection -- 9.0 instead of 2.3 at 50 000 rows)
      unsigned long long mk = __ballot(t[i] == wmax && ((have >> i) & 1u) != 0u);
      while (mk) {
        const uint32_t k = (uint32_t)slice * FG_P + wave_base + (uint32_t)__builtin_ctzll(mk) + (uint32_t)(i * FG_THREADS);
        mk &= mk - 1ull;
        const uint32_t tk = ~fps_tie_key(k, lg, bs);
        btk = tk > btk ? tk : btk;
      }
    }
    if (lane == 0) atomicMax(&s_best[cur], ((unsigned long long)wmax << 32) | btk);
    if (tid == 0) s_best[nxt] = 0ull;
    __syncthreads();
    unsigned long long w = s_best[cur];
    cur = nxt;
    nxt = nxt == 2 ? 0 : nxt + 1;
    if (G > 1) {                                     // (uniform over the workgroup)
      if (tid == 0) {
        fg_gu64* slot = slots + (j % 3);
        (void)__hip_atomic_fetch_max(slot, w, FG_RLX_AGENT);
        if (slice == 0) (void)__hip_atomic_exchange(slots + ((j + 1) % 3), 0ull, FG_RLX_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // post and clear acknowledged before the arrival can be seen
        (void)__hip_atomic_fetch_add(cnt, 1ull, FG_RLX_AGENT);
        const bool ok = fg_wait(cnt, (unsigned long long)G * (unsigned long long)j, status);
        s_win = ok ? __hip_atomic_load(slot, FG_RLX_AGENT) : 0ull;
        s_ok = ok ? 1 : 0;
      }
      __syncthreads();
      if (!s_ok) {
        for (int q = j + tid; q < mreq; q += FG_THREADS) out[q] = -1;
        return;
      }
      w = s_win;
    }
    old = max(0, min(fps_decode(~(uint32_t)w, lg), len - 1));    // (the clamp cannot bind on a sound key: it keeps the centre read in range whatever a slot holds)
    old = __builtin_amdgcn_readfirstlane(old);
    if (slice == 0 && tid == 0) out[j] = rel + old;
  }
}
