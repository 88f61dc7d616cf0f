// The text of zx4_kernel and zx4_rows_kernel (mmx_fused4.hip, which has the design notes): included into either body,
// which states NKX, LA, InT, Q16, NTW, ELDS and ROWS.
    using cg = cls4<NKX, LA>;
    using pc = pieces4<InT>;
    constexpr int NKZ = cg::NKZ, NT = cg::NT;
    constexpr bool SPLIT = cg::SPLIT;                 // radius > 16: operand slot 0 of the Z pass is the split tile (cls4)
    constexpr int kUnit = std::is_same<InT, float>::value ? 512 : 256;      // bytes of a unit of the voxel copy
    constexpr bool LO_SCALED = lo_scaled4<InT>::value;
    static_assert(NTW == 1 || (NTW == 2 && Q16 && NKX == 2 && LA == 1), "two tiles per wave: 16-bit tiles, 8 < radius <= 16");
    // radius <= 16: the Z fragments of the interior z tiles live in LDS, shared by the workgroup's waves, and
    // two z tiles are in flight instead of three: 154 registers, three waves per SIMD.  (Radius > 16, measured when
    // it still had three k-steps of Z fragments: with float32 tiles, which are bound by their stores, fetching them
    // from LDS every step cost more than the third wave gave -- 4.19 against 3.87 ms --; with 16-bit tiles it paid:
    // 3.10 against 3.15 ms.)
    constexpr bool ZLDS = LA == 1 || Q16;
    constexpr int PF = ZLDS ? ZX6_PF : kPF4;         // z tiles of voxels in flight per wave
    // ROWS (the pair kernel's LDS form): a wave owns its column pair over NR consecutive rows of its block and marches
    // through them as one row of NR ntz z tiles -- the copy's row tiles of row y + 1 follow those of row y --: one table
    // fill, one set of X fragments and start values, one X-only head and one clamped tail per NR rows.  Flat grid.
    [[maybe_unused]] zx4_rows_place place{};
    if constexpr (ROWS) place = zx4_rows_decode(zx4_sched_of(cfg), (int)blockIdx.x);
    const mmx_block bd = blocks[ROWS ? (unsigned)place.block : blockIdx.y];
    const int W = bd.nx, nz = bd.nz;
    const int ntx = (W + 15) >> 4;
    // (readfirstlane: the wave index is uniform, but only this tells the compiler -- otherwise every buffer
    //  descriptor below is built per lane and each load becomes a waterfall loop)
    // workgroups are dealt to the 8 XCDs round robin; neighbours along x read overlapping windows, so the
    // workgroups one XCD gets (every 8th) are made neighbours: its L2 then serves the overlap (gridDim.x % 8 == 0)
    const int bx = ROWS ? (place.wx & 7) * (place.wgs >> 3) + (place.wx >> 3)
                        : (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int gw = bx * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave of this block: (y, column)
    const int ntp = (ntx + NTW - 1) / NTW;                      // waves per row: one per tile, or per pair of tiles
    // (ROWS: y is the first row of the wave's run of nrw <= NR rows)
    const int y = ROWS ? (gw / ntp) * place.n : gw / ntp;
    const int c = (gw - (gw / ntp) * ntp) * NTW;                // (first) column tile of this wave
    [[maybe_unused]] const int nrw = bd.ny - y < place.n ? bd.ny - y : place.n;
    const int lane = threadIdx.x & 63;
    const int li = lane & 15, kq = lane >> 4;
    [[maybe_unused]] const bool lowk = kq < 2;                  // this lane holds planes 0 .. 7 of a tile's 16 as a Z operand
    int cw = 0, cz = 0;
    for (int i = 1; i < cfg.ncw; ++i) cw = cfg.wcls[i] == W ? i : cw;
    for (int i = 1; i < cfg.ncz; ++i) cz = cfg.zcls[i] == nz ? i : cz;
    const int ntz = (nz + 15) >> 4;
    const int ntl = ROWS ? nrw * ntz : ntz;                     // z tiles the wave loads: of all its rows, one after the other
    const int R = cfg.radius;
    const int u_lo = (R + 15) >> 4;                             // first U with 16 U - R >= 0
    const int u_hi = (nz - 16 - R) >> 4;                        // last U with 16 U + 15 + R <= nz - 1 (may be < u_lo)
    const v4u* zt = ztab + ((size_t)cz * cfg.maxu * NKZ * 2) * 128 + lane;
    // (the steps at the ends of the block take their fragments straight from the table)
    // ROT: in the steady steps z tile t keeps the window slot t mod NT it was written to -- no shifting, the operand
    // quads (slots 2 q, 2 q + 1) never move -- and the fragments rotate instead: by whole k-steps when the window
    // starts on an even slot (the table as it is), and through a second table, shifted by one tile, when it starts on
    // an odd one: F1[k] = [F0[k - 1] upper half | F0[k] lower half].  The slot outside the window holds the tile that
    // left it (finite values) against zero fragments.  A third fewer register moves per step; built where it measured
    // faster (tools/kbench.py, 16-bit tiles, ms per 22 blocks: radius 8 0.752 -> 0.70, radius 18 / 20 1.02 -> 0.975);
    // two column tiles per wave spill with it (76 bytes: 0.75 -> 1.20), one tile per wave at radius 9..16 loses to
    // the pair as before (0.845 against 0.74), float32 tiles read +6 %: profiles/r05_experiments.txt, section 6.
    // Radius > 16 (SPLIT): the four slots hold z tiles t - 4 .. t - 1 whole; the X results of z tile t stay in registers
    // of their own during the step, the split tile is chosen per lane between them and slot t mod 4 (z tile t - 4),
    // and they become that slot once the Z pass has read it.  The slot of the split tile goes round with t, the quads
    // never move, and the shifted table is the cyclic one: F1[k] = [F0[k - 1 mod 2] upper half | F0[k] lower half].
    constexpr bool ROT = ZLDS && Q16 && NTW == 1 && !is_f32_4<InT>::value && (NKX == 1 || LA == 2);
    constexpr int ZL1 = NKZ * 4 * 64;                          // entries of one table
    // EDGE: the tables of the block's edge output tiles (U < u_lo, U > u_hi) stand in LDS too, behind the interior one(s),
    // in slots 0 .. nE - 1: the low tiles first, then the high ones from hi0 on.  A workgroup's four waves belong to one
    // block, so one set serves them all, and no step of the march waits for a load it has issued itself: the steps
    // outside the steady loop have the steady form's memory instructions -- one tile of voxels in, the results out -- and
    // take their fragments from LDS at an address that is a run-time scalar.  kMaxEdge bounds nE for every depth of the
    // class but those that leave radius 18 .. 24 a third high tile (nz mod 16 in [1, R - 16)) or no interior tile among
    // five.  ELDS is a kernel of its own (one head and one tail per kernel: both forms in one spill): launch_zx6 takes it
    // when every depth class of the batch fits (zx4_edge_tiles) and MMX_ZX_EDGE_GLOBAL is not set, and the kernel whose
    // edge steps read the global table otherwise.
    constexpr bool EDGE = ELDS;
    static_assert(!ELDS || (ZLDS && Q16 && !is_f32_4<InT>::value), "LDS edge tables: 16-bit tiles of integer voxels");
    constexpr int MAXE = EDGE ? cg::kMaxEdge : 0;
    constexpr int ZE0 = (ROT ? 2 : 1) * ZL1;                   // first entry of the edge tables
    const int hi0 = zx4_edge_tiles(nz, R).hi0;                 // first high edge tile
    __shared__ v4u zl[ZLDS ? ZE0 + MAXE * ZL1 : 1];
    if constexpr (ZLDS) {
        const v4u* zi = ztab + ((size_t)(cz * cfg.maxu + (u_lo < cfg.maxu ? u_lo : 0)) * NKZ * 2) * 128;
        if constexpr (EDGE) {
            // every load of the fill in flight before the first LDS write (slots past nE: the last z tile again)
            const v4u* zc = ztab + ((size_t)(cz * cfg.maxu) * NKZ * 2) * 128;     // table of z tile 0 of this depth class
            v4u f[MAXE + 1][ZL1 / 256];
#pragma unroll
            for (int sl = 0; sl <= MAXE; ++sl) {
                int tile = sl - 1 < u_lo ? sl - 1 : hi0 + (sl - 1 - u_lo);
                tile = tile < ntz - 1 ? tile : ntz - 1;
                const v4u* src = sl ? zc + ((size_t)tile * NKZ * 2) * 128 : zi;
#pragma unroll
                for (int j = 0; j < ZL1 / 256; ++j) f[sl][j] = src[threadIdx.x + 256 * j];
            }
#pragma unroll
            for (int sl = 0; sl <= MAXE; ++sl)
#pragma unroll
                for (int j = 0; j < ZL1 / 256; ++j) zl[(sl ? ZE0 + (sl - 1) * ZL1 : 0) + threadIdx.x + 256 * j] = f[sl][j];
        } else {
            for (int e = threadIdx.x; e < ZL1; e += 256) zl[e] = zi[e];
        }
        __syncthreads();
        if constexpr (ROT) {
            for (int e = threadIdx.x; e < ZL1; e += 256) {
                const v4u cur = zl[e];
                // (k-step before: 4 x 64 entries back; the split tile's window is a ring -- its first k-step follows its last)
                const v4u prev = SPLIT ? zl[(e + ZL1 - 256) % ZL1] : (e >= 256 ? zl[e - 256] : (v4u){0u, 0u, 0u, 0u});
                zl[ZL1 + e] = (v4u){prev.z, prev.w, cur.x, cur.y};
            }
            __syncthreads();
        }
    }
    if (y >= bd.ny) return;                                   // whole wave (no barriers below)

    // LDS form: the first PF voxel tiles go out here (load_tile's addresses, below), ahead of the X fragment loads
    [[maybe_unused]] typename pc::raw_t raw_early[ELDS ? PF : 1][NKX];
    if constexpr (ELDS) {
        const rsrc_t rin0 = make_rsrc(vol + (int64_t)bd.slot * stride_z);
        const int nch0 = (W + 7) >> 3;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const unsigned so = (unsigned)((y * ntz + (u < ntl ? u : ntl - 1)) * nch0) * (unsigned)kUnit;
#pragma unroll
            for (int m = 0; m < NKX; ++m) {
                int j = 2 * c - cg::R8 / 8 + 4 * m + kq;
                j = j < 0 ? 0 : (j > nch0 - 1 ? nch0 - 1 : j);
                raw_early[u][m] = pc::load(rin0, (unsigned)(j * kUnit + li * 16), so);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    // X fragments of this wave's column tile(s): [tile][m][kernel][piece]
    v4u xw[NTW][NKX][2][2];
    const bool has2 = NTW == 2 && c + 1 < ntx;                 // (wave-uniform)
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        // (a pair's missing second tile: any column's fragments -- its results are never stored)
        const v4u* xt = xtab + ((size_t)(cw * cfg.maxcol + (i && !has2 ? c : c + i)) * NKX * 2) * 128 + lane;
#pragma unroll
        for (int m = 0; m < NKX; ++m)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                xw[i][m][k][0] = xt[(m * 2 + k) * 128];
                xw[i][m][k][1] = xt[(m * 2 + k) * 128 + 64];
            }
    }
    // 16-bit tiles: the voxel pieces keep their exponent offsets (pieces4::split_biased) and the X accumulators start
    // at minus what the offsets add -- (offset x column sum of the fragments), the same for the four rows a lane holds.
    // The sums come from the matrix cores themselves: an A operand of ones.  Their float32 rounding (values of ~5
    // instead of <= 1: 5e-7) is inside what mmx_tiled_q16_error_bound states.
    // (radius > 16: the eight start registers would push the kernel past three waves per SIMD)
    constexpr bool BIASED = Q16 && !is_f32_4<InT>::value && LA == 1;
    constexpr bool MIXSPLIT = Q16;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
    v4f a_start[NTW], b_start[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) { a_start[i] = zero4; b_start[i] = zero4; }
    if constexpr (BIASED) {
        const v4u ones = {0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u};
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            v4f sh[2] = {zero4, zero4}, sl[2] = {zero4, zero4};
#pragma unroll
            for (int m = 0; m < NKX; ++m)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    sh[k] = mfma16(ones, xw[i][m][k][0], sh[k]);
                    sl[k] = mfma16(ones, xw[i][m][k][1], sl[k]);
                }
            // a0 takes (hi + lo pieces) x high fragments, a1 hi pieces x low fragments (scaled by 2048), v = a0 + a1 / 2048
            const float ca = -((pc::kBiasHi + pc::kBiasLo) * sh[0][0] + pc::kBiasHi * sl[0][0] * kLoInv);
            const float cb = -((pc::kBiasHi + pc::kBiasLo) * sh[1][0] + pc::kBiasHi * sl[1][0] * kLoInv);
            a_start[i] = (v4f){ca, ca, ca, ca};
            b_start[i] = (v4f){cb, cb, cb, cb};
        }
    }
    // Z fragments: [ks][kernel][piece], of the z tile being produced (reloaded when its class changes);
    // interior z tiles share one set: the first tile whose taps all fall inside the block
    v4u zw[ZLDS ? 1 : NKZ][2][2];
    int zset = -1;

    // voxel rows: plane z0 + li, chunk of 8 x at xl[m] (clamped into the block; the fragments know)
    const InT* in = vol + (int64_t)bd.slot * stride_z;
    const int nch8 = (W + 7) >> 3;                               // 256-byte units (8 columns x 16 planes) per row tile
    unsigned xoff[NKX];
#pragma unroll
    for (int m = 0; m < NKX; ++m) {
        int j = 2 * c - cg::R8 / 8 + 4 * m + kq;                 // unit of this lane; outside the row: any unit, zero weights
        j = j < 0 ? 0 : (j > nch8 - 1 ? nch8 - 1 : j);
        xoff[m] = (unsigned)(j * kUnit + li * 16);
    }
    const rsrc_t rin = make_rsrc(in);
    auto load_tile = [&](int t, typename pc::raw_t (&raw)[NKX]) __attribute__((always_inline)) {
        const unsigned so = (unsigned)((y * ntz + t) * nch8) * (unsigned)kUnit;          // wave-uniform: the row tile
#pragma unroll
        for (int m = 0; m < NKX; ++m) raw[m] = pc::load(rin, xoff[m], so);
    };

    // window of X results as float16 pieces: [column tile][array: A hi, A lo, B hi, B lo][z tile][2 dwords]
    unsigned win[NTW][4][NT][2];
#pragma unroll
    for (int w = 0; w < NTW; ++w)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < NT; ++i) { win[w][a][i][0] = 0u; win[w][a][i][1] = 0u; }

    // One descriptor per wave, over the tile column (y, c, all U) it writes -- ntz KiB -- and ENDING where the
    // block's planes end: the rows of the last z tile past the block (11 of 16 at 261 planes) fall outside it and the
    // hardware drops their part of the store, 4 % of the kernel's write requests, without a branch or an exec mask.
    // Nothing reads them: the Y pass works within a plane and discards the planes past the block (ym_kernel: `real`).
    // (Second tile of a pair: the next ntz KiB, 0 records when the row has no such tile -- its stores are dropped.)
    const unsigned col_b = (unsigned)ntz * 1024u;                                        // bytes of one tile column
    const unsigned live_b = col_b - (unsigned)(16 * ntz - nz) * 64u;
    const int64_t wave_e = (int64_t)((y * ntx + c) * ntz) * 256;                          // elements before this wave's tiles
    // (ROWS: of the row whose tiles the march is storing -- rebuilt on the scalar side, below)
    rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(gp + (int64_t)bd.slot * slot_elems + wave_e, 0, (int)live_b, 0x00020000);
    const rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(gq + (int64_t)bd.slot * slot_elems + wave_e, 0, (int)live_b, 0x00020000);
    rsrc_t rp2 = __builtin_amdgcn_make_buffer_rsrc(gp + (int64_t)bd.slot * slot_elems + wave_e + (int64_t)ntz * 256, 0,
                                                    has2 ? (int)live_b : 0, 0x00020000);
    // Tile (y, c, U) of 16 z x 16 x floats, row-major, at ((y ntx + c) ntz + U) KiB: what a wave writes
    // during its march is contiguous, the waves of a workgroup and the workgroups of a row follow each other --
    // the kernel's stores are one sequential stream -- and y6_kernel's workgroups, one per (c, U), all read inside
    // the same ntx ntz KiB at any time.  (Measured against the (c, U, y) order: no difference in either kernel; both
    // run at the request rate the memory system sustains, DESIGN.md section 4b.)
    const unsigned plane_b = 64u;
    unsigned obase = (unsigned)((4 * li + kq) * 16);                  // (relative to the wave's tile column)

    // voxels of the next ZX4_PF z tiles, in flight.  vmcnt counts loads and stores together and in issue order:
    // a tile loaded only one step ahead could not be used before the stores of the step in between have been
    // acknowledged by L2 -- measured, that wait and not the arithmetic set the step time (5.3 ms against 2.1 ms
    // without the stores).  With PF steps of distance the stores older than the tile being consumed have had
    // PF - 1 whole steps to complete.
    // (LDS form: issued before the X fragments are loaded and waited for -- the BIASED start values need them at once
    //  --, so that the two latencies overlap; the other kernels measured 0.4 .. 1.3 % slower with it and issue them here
    //  as before: profiles/r14_zx_edge_steps.txt, section 4)
    typename pc::raw_t raw[PF][NKX];
    constexpr bool EARLY = ELDS;
    if constexpr (EARLY) {
#pragma unroll
        for (int u = 0; u < PF; ++u)
#pragma unroll
            for (int m = 0; m < NKX; ++m) raw[u][m] = raw_early[u][m];
    } else {
#pragma unroll
        for (int u = 0; u < PF; ++u) load_tile(u < ntz ? u : ntz - 1, raw[u]);
    }

    // One march step: X pass of z tile t into the window, Z pass of z tile t - LA out of it.  STEADY = the
    // branch-free form for the tiles in the middle of the block (every tile real, interior Z fragments already
    // in registers, every output plane real): with no control flow between the memory instructions the
    // compiler's s_waitcnt vmcnt(N) are exact counts and only ever wait for the tile being consumed.
    // Results on their way to memory: a store reads its data registers asynchronously, so the compiler makes the
    // next writer of those registers wait (vmcnt) until the store has completed.  Each ring slot therefore has
    // its own result registers, kept allocated (an empty asm "use") until the slot comes round again.
    v4f outP[PF][NTW], outQ[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
#pragma unroll
        for (int w = 0; w < NTW; ++w) outP[u][w] = zero4;
        outQ[u] = zero4;
    }
    // (phase_tag: the window slot of z tile t in a steady step of the rotating form, -1 otherwise: the window is
    //  shifted and t takes slot 2 LA -- the arrangement the rotating steps start from and return to every NT steps)
    // (form_tag: 0 = as the other tags say; 1, 2 = a step outside the steady loop in the LDS form (EDGE): the voxel
    //  loads and the X pass as in a steady step -- past the last z tile the clamped tile again, whose results meet zero
    //  weights: the voxel pieces are finite numbers, 0 x finite = 0 --, 1: no Z pass (the first LA steps), 2: the Z pass
    //  of z tile t - LA, a real one, with the fragments at entry zb of the LDS tables)
    auto step = [&](int t, auto steady_tag, auto phase_tag, typename pc::raw_t (&rw)[NKX], v4f (&P)[NTW], v4f& Q,
                    auto form_tag, int zb) __attribute__((always_inline)) {
        constexpr bool STEADY = decltype(steady_tag)::value;
        constexpr int PH = decltype(phase_tag)::value;
        constexpr int FORM = decltype(form_tag)::value;
        constexpr bool NOBR = STEADY || FORM != 0;               // no branch around a memory instruction
        constexpr bool TURN = STEADY && ROT && PH >= 0;
        constexpr int SLOT = TURN ? PH : 2 * LA;                 // where the X results of z tile t go
        // SPLIT: they go to xr, and into the window after the Z pass; VS = the slot of z tile t - 4, which the split
        // tile shares with them (0 in the shifting form: the slots hold z tiles t - 4 .. t - 1)
        constexpr int VS = TURN ? PH : 0;
        unsigned xr[4][2] = {{0u, 0u}, {0u, 0u}, {0u, 0u}, {0u, 0u}};
        auto put = [&](int w, int a, int d, unsigned v) __attribute__((always_inline)) {
            if constexpr (SPLIT) xr[a][d] = v;
            else win[w][a][SLOT][d] = v;
        };
        if constexpr (!TURN && !SPLIT) {
            // shift the window by one z tile
#pragma unroll
            for (int w = 0; w < NTW; ++w)
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int i = 0; i < 2 * LA; ++i) { win[w][a][i][0] = win[w][a][i + 1][0]; win[w][a][i][1] = win[w][a][i + 1][1]; }
        }
        if (NOBR || t < ntz) {
            // ---- X pass of z tile t
            v4u dh[NKX], dl[NKX];
#pragma unroll
            for (int m = 0; m < NKX; ++m) {
                if constexpr (BIASED) pc::split_biased(rw[m], dh[m], dl[m]);
                else pc::split(rw[m], dh[m], dl[m]);
            }
            // (past the last tile the ring re-reads it: loads without a branch, never used)
            // the scheduler must not sink these loads to the end of the unrolled ring (it does, given the chance:
            // all of a ring's loads then sit right in front of their first use)
            __builtin_amdgcn_sched_barrier(0);
            if (NOBR) load_tile(t + PF < ntl ? t + PF : ntl - 1, rw);
            else if (t + PF < ntz) load_tile(t + PF, rw);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int w = 0; w < NTW; ++w) {
                v4f a0 = a_start[w], a1 = zero4, b0 = b_start[w], b1 = zero4;
#pragma unroll
                for (int m = 0; m < NKX; ++m) {
                    a0 = mfma16(dh[m], xw[w][m][0][0], a0);
                    b0 = mfma16(dh[m], xw[w][m][1][0], b0);
                    a1 = mfma16(dh[m], xw[w][m][0][1], a1);
                    b1 = mfma16(dh[m], xw[w][m][1][1], b1);
                    if constexpr (LO_SCALED) {
                        // (float voxels: the low piece carries x 2048 like the low fragments; low x low is 2^-22 of a product)
                        a1 = mfma16(dl[m], xw[w][m][0][0], a1);
                        b1 = mfma16(dl[m], xw[w][m][1][0], b1);
                    } else {
                        a0 = mfma16(dl[m], xw[w][m][0][0], a0);
                        b0 = mfma16(dl[m], xw[w][m][1][0], b0);
                        // (low voxel byte x low weight piece: <= 2^-19 of a product.  The float32 tiles keep it; the 16-bit
                        //  tiles' error bound has room for it: mmx_tiled_q16_error_bound counts 1.9e-6 per X sum)
                        if constexpr (!Q16) {
                            a1 = mfma16(dl[m], xw[w][m][0][1], a1);
                            b1 = mfma16(dl[m], xw[w][m][1][1], b1);
                        }
                    }
                }
                // combine the two accumulators and split into float16 pieces: v = acc0 + acc1 / 2048
#pragma unroll
                for (int r = 0; r < 4; r += 2) {
                    const float av0 = __builtin_fmaf(a1[r], kLoInv, a0[r]), av1 = __builtin_fmaf(a1[r + 1], kLoInv, a0[r + 1]);
                    const float bv0 = __builtin_fmaf(b1[r], kLoInv, b0[r]), bv1 = __builtin_fmaf(b1[r + 1], kLoInv, b0[r + 1]);
                    const v2f av = {av0, av1}, bv = {bv0, bv1};
                    const v2h ah = __builtin_convertvector(av, v2h), bh = __builtin_convertvector(bv, v2h);
                    if constexpr (MIXSPLIT) {
                        // 16-bit tiles: the low piece is the plain residual v - half(v), not scaled by 2048 -- values are
                        // <= 1 here (the fragments carry 1 / bound), so the residual is below 2^-12 and float16 keeps it to
                        // 2^-24 absolute, a 250th of the 16-bit quantum; the Z pass below adds it at full weight.
                        // (v_fma_mix{lo,hi}_f16 would make it in one instruction per value, but only as inline assembly,
                        //  whose register writes the compiler's hazard recogniser does not see: one landed right behind an
                        //  MFMA that still read the register as its C operand -- wrong results for radius <= 8.)
                        const v2f ar = {av0 - (float)ah.x, av1 - (float)ah.y}, br = {bv0 - (float)bh.x, bv1 - (float)bh.y};
                        put(w, 0, r >> 1, __builtin_bit_cast(unsigned, ah));
                        put(w, 1, r >> 1, __builtin_bit_cast(unsigned, __builtin_convertvector(ar, v2h)));
                        put(w, 2, r >> 1, __builtin_bit_cast(unsigned, bh));
                        put(w, 3, r >> 1, __builtin_bit_cast(unsigned, __builtin_convertvector(br, v2h)));
                        continue;
                    }
                    const v2f ar = {__builtin_fmaf((float)ah.x, -kLoScale, av0 * kLoScale), __builtin_fmaf((float)ah.y, -kLoScale, av1 * kLoScale)};
                    const v2f br = {__builtin_fmaf((float)bh.x, -kLoScale, bv0 * kLoScale), __builtin_fmaf((float)bh.y, -kLoScale, bv1 * kLoScale)};
                    put(w, 0, r >> 1, __builtin_bit_cast(unsigned, ah));
                    put(w, 1, r >> 1, __builtin_bit_cast(unsigned, __builtin_convertvector(ar, v2h)));
                    put(w, 2, r >> 1, __builtin_bit_cast(unsigned, bh));
                    put(w, 3, r >> 1, __builtin_bit_cast(unsigned, __builtin_convertvector(br, v2h)));
                }
            }
        } else {
#pragma unroll
            for (int w = 0; w < NTW; ++w)
#pragma unroll
                for (int a = 0; a < 4; ++a) { put(w, a, 0, 0u); put(w, a, 1, 0u); }
        }
        const int U = t - LA;
        if (FORM != 1 && (NOBR || U >= 0)) {
            // ---- Z pass of z tile U
            const int want = (U >= u_lo && U <= u_hi) ? u_lo : U;
            if constexpr (!STEADY && !ZLDS) {
                if (want != zset) {
                    zset = want;
#pragma unroll
                    for (int ks = 0; ks < NKZ; ++ks)
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            zw[ks][k][0] = zt[((size_t)(want * NKZ + ks) * 2 + k) * 128];
                            zw[ks][k][1] = zt[((size_t)(want * NKZ + ks) * 2 + k) * 128 + 64];
                        }
                }
            }
            // the split tile: the lower half of z tile t where this lane holds planes 0 .. 7 of a tile, the upper half of
            // z tile t - 4 where it holds planes 8 .. 15 (eight selects, nothing crosses lanes)
            unsigned vsel[4][2];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                vsel[a][0] = SPLIT ? (lowk ? xr[a][0] : win[0][a][VS][0]) : 0u;
                vsel[a][1] = SPLIT ? (lowk ? xr[a][1] : win[0][a][VS][1]) : 0u;
            }
            auto wv = [&](int w, int a, int s, int d) __attribute__((always_inline)) {
                return SPLIT && s == VS ? vsel[a][d] : win[w][a][s][d];
            };
            v4f p0[NTW], p1[NTW], q0[NTW], q1[NTW];
#pragma unroll
            for (int w = 0; w < NTW; ++w) { p0[w] = zero4; p1[w] = zero4; q0[w] = zero4; q1[w] = zero4; }
#pragma unroll
            for (int ks = 0; ks < NKZ; ++ks) {
                v4u z00, z01, z10, z11;          // [kernel][piece]
                if constexpr (!ZLDS) {
                    z00 = zw[ks][0][0]; z01 = zw[ks][0][1]; z10 = zw[ks][1][0]; z11 = zw[ks][1][1];
                } else if constexpr (STEADY) {
                    // (rotating form: the window starts TR slots after slot 0; quad ks holds the window tiles of k-step
                    //  ks - TR / 2, one tile later when TR is odd)
                    //  (SPLIT: the split tile's slot is TR itself -- quad ks holds k-step ks + TR / 2 mod 2 of the table, or of
                    //   the cyclically shifted one when TR is odd)
                    constexpr int TR = TURN ? (SPLIT ? PH : (PH - (NT - 2) + NT) % NT) : 0;
                    const int KF = ((TR & 1) ? ZL1 : 0) + ((ks - TR / 2 + NKZ) % NKZ) * 256;     // (a constant once unrolled)
                    z00 = zl[KF + 0 * 64 + lane]; z01 = zl[KF + 1 * 64 + lane];
                    z10 = zl[KF + 2 * 64 + lane]; z11 = zl[KF + 3 * 64 + lane];
                } else if constexpr (FORM == 2) {
                    const int KF = zb + ks * 256 + lane;
                    z00 = zl[KF + 0 * 64]; z01 = zl[KF + 1 * 64];
                    z10 = zl[KF + 2 * 64]; z11 = zl[KF + 3 * 64];
                } else {
                    const v4u* zp = zt + ((size_t)(want * NKZ + ks) * 2) * 128;
                    z00 = zp[0]; z01 = zp[64]; z10 = zp[128]; z11 = zp[192];
                }
                // (Radius <= 16: the window's last tile, U + 1, stands alone in its k-step -- the fragments' other half is
                //  zero.  The legacy v_mfma_f32_16x16x16_f16 on that half costs what the 16x16x32 form costs on gfx950 and,
                //  mixed with it on one accumulator chain, gave run-dependent values: profiles/r05_experiments.txt, section 5.)
#pragma unroll
                for (int w = 0; w < NTW; ++w) {
                    const v4u ah = {wv(w, 0, 2 * ks, 0), wv(w, 0, 2 * ks, 1), wv(w, 0, 2 * ks + 1, 0), wv(w, 0, 2 * ks + 1, 1)};
                    const v4u al = {wv(w, 1, 2 * ks, 0), wv(w, 1, 2 * ks, 1), wv(w, 1, 2 * ks + 1, 0), wv(w, 1, 2 * ks + 1, 1)};
                    const v4u bh = {wv(w, 2, 2 * ks, 0), wv(w, 2, 2 * ks, 1), wv(w, 2, 2 * ks + 1, 0), wv(w, 2, 2 * ks + 1, 1)};
                    const v4u bl = {wv(w, 3, 2 * ks, 0), wv(w, 3, 2 * ks, 1), wv(w, 3, 2 * ks + 1, 0), wv(w, 3, 2 * ks + 1, 1)};
                    p0[w] = mfma16(ah, z00, p0[w]);
                    q0[w] = mfma16(bh, z00, q0[w]);
                    p1[w] = mfma16(ah, z01, p1[w]);
                    q1[w] = mfma16(bh, z01, q1[w]);
                    if constexpr (MIXSPLIT) {          // (unscaled low pieces: into the full-weight accumulators)
                        p0[w] = mfma16(al, z00, p0[w]);
                        q0[w] = mfma16(bl, z00, q0[w]);
                    } else {
                        p1[w] = mfma16(al, z00, p1[w]);
                        q1[w] = mfma16(bl, z00, q1[w]);
                    }
                    q0[w] = mfma16(ah, z10, q0[w]);
                    q1[w] = mfma16(ah, z11, q1[w]);
                    if constexpr (MIXSPLIT) q0[w] = mfma16(al, z10, q0[w]);
                    else q1[w] = mfma16(al, z10, q1[w]);
                }
                if constexpr (ZLDS && !STEADY && FORM == 0) __builtin_amdgcn_sched_barrier(0);    // one k-step's fragments at a time
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int w = 0; w < NTW; ++w) asm volatile("" ::"v"(P[w]));     // the slot's previous results stayed in these registers until now
            // (16-bit tiles never write Q; at radius > 16 the registers this would pin are the ones the kernel lacks)
            if constexpr (!(Q16 && SPLIT)) asm volatile("" ::"v"(Q));
            {                                           // (a tile is stored whole: its padding belongs to it)
                // the results reach the slot's registers through opaque moves: the stores then read registers
                // that nothing else may be allocated to before the slot comes round again
                if constexpr (Q16) {
#pragma unroll
                    for (int w = 0; w < NTW; ++w) {
#pragma unroll
                        for (int r = 0; r < 4; r += 2) {
                            const float pa = __builtin_fmaf(p1[w][r], kLoInv, p0[w][r]), pb = __builtin_fmaf(p1[w][r + 1], kLoInv, p0[w][r + 1]);
                            const float qa = __builtin_fmaf(q1[w][r], kLoInv, q0[w][r]), qb = __builtin_fmaf(q1[w][r + 1], kLoInv, q0[w][r + 1]);
                            const unsigned pu = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pknorm_u16(pa, pb));   // [Pa | Pb]
                            const unsigned qs = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pknorm_i16(qa, qb));   // [Qa | Qb]
                            const unsigned da = __builtin_amdgcn_perm(qs, pu, 0x05040100u);     // [Pa | Qa]
                            const unsigned db = __builtin_amdgcn_perm(qs, pu, 0x07060302u);     // [Pb | Qb]
                            float ra, rb;
                            asm volatile("v_mov_b32 %0, %1" : "=v"(ra) : "v"(__uint_as_float(da)));
                            asm volatile("v_mov_b32 %0, %1" : "=v"(rb) : "v"(__uint_as_float(db)));
                            P[w][r] = ra;
                            P[w][r + 1] = rb;
                        }
                        // (tile (y, c + w, U) lies ntz KiB after tile (y, c, U): rp2's base)
                        if (w == 0) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, P[w]), rp, obase, 0, ZX4_ST_AUX);
                        else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, P[w]), rp2, obase, 0, ZX4_ST_AUX);
                    }
                } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pv = __builtin_fmaf(p1[0][r], kLoInv, p0[0][r]);
                    const float qv = __builtin_fmaf(q1[0][r], kLoInv, q0[0][r]);
                    float pr, qr;
                    asm volatile("v_mov_b32 %0, %1" : "=v"(pr) : "v"(pv));
                    asm volatile("v_mov_b32 %0, %1" : "=v"(qr) : "v"(qv));
                    P[0][r] = pr;
                    Q[r] = qr;
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, P[0]), rp, obase, 0, ZX4_ST_AUX);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, Q), rq, obase, 0, ZX4_ST_AUX);
                }
            }
            obase += 16u * plane_b;
        }
        if constexpr (FORM == 1) {
            // no output tile yet (U < 0): the step still issues its stores, at an offset past any tile column, where the
            // descriptor's range drops them like the rows past the block -- every step of the march then has the same
            // memory instructions, the compiler's vmcnt counts at the head of the steady loop are the steady state's own,
            // and nothing has to be drained in front of it
            constexpr unsigned kDropped = 0x80000000u;          // (a tile column is below 2^31 bytes: mmx_zx6_plan_make)
#pragma unroll
            for (int w = 0; w < NTW; ++w) {
                if (w == 0) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, P[w]), rp, kDropped, 0, ZX4_ST_AUX);
                else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, P[w]), rp2, kDropped, 0, ZX4_ST_AUX);
            }
        }
        if constexpr (SPLIT) {
            // z tile t takes its place in the window: the slot of z tile t - 4 where the slots stay, the last one where
            // they shift
            if constexpr (!TURN) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int i = 0; i < NT - 1; ++i) { win[0][a][i][0] = win[0][a][i + 1][0]; win[0][a][i][1] = win[0][a][i + 1][1]; }
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) { win[0][a][TURN ? PH : NT - 1][0] = xr[a][0]; win[0][a][TURN ? PH : NT - 1][1] = xr[a][1]; }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // tiles [0, tA): generic steps up to the first interior output tile (U = t - LA >= u_lo), rounded up to a
    // multiple of the ring; [tA, tB): steady steps (U in [u_lo, u_hi], t < ntz), whole rings; the rest generic.
    const int t_end = ntz + LA;
    int tA = ((u_lo + LA + PF - 1) / PF) * PF;
    int nB = (u_hi + LA + 1 < ntz ? u_hi + LA + 1 : ntz) - tA;       // steady steps available
    constexpr int GROUP = ROT ? NT : PF;                             // (rotating form: whole turns of the window)
    static_assert(GROUP % PF == 0, "a turn of the window is a whole number of rings");
    nB = nB > 0 ? (nB / GROUP) * GROUP : 0;
    if (tA > t_end) tA = ((t_end + PF - 1) / PF) * PF;
    const int tB = tA + nB;
    // LDS form: the head is straight-line code -- u_lo == LA in every class, so tA == 2 LA and the head is LA steps of X
    // alone, then the low edge tiles U = 0 .. LA - 1 from slots 0 .. LA - 1 -- and every block has that many steps
    // (zx4_edges_fit)
    [[maybe_unused]] auto edge_step = [&](int t, auto u_tag, auto form_tag, int zb) __attribute__((always_inline)) {
        constexpr int u = decltype(u_tag)::value;
        step(t, std::false_type{}, std::integral_constant<int, -1>{}, raw[u], outP[u], outQ[u], form_tag, zb);
    };
    if constexpr (ROWS) {
        // One march over the wave's linear tile index g = 0 .. ntl: step g loads tile min(g + PF, ntl - 1), does the X
        // pass of tile g (past the last one: the clamped tile) and the Z pass of tile g - 1 -- output tile U = (g - 1) mod
        // ntz of row y + (g - 1) / ntz -- with the table of U at a run-time LDS address: the interior one for u_lo <= U <=
        // u_hi, the edge slots otherwise.  The edge tables carry zero weights for the slots outside the block, so what
        // stands there at a row change -- the last tile of the row above, the first of the row below -- adds nothing
        // (finite pieces x 0), as the zeroed window and the clamped tile do at the two ends of the march.  Every step has
        // the steady step's memory instructions; the store descriptors and the tile's offset follow U on the scalar side.
        using std::integral_constant;
        static_assert(PF == 2 && LA == 1, "the row march is written for a ring of two and one step of look-ahead");
        const unsigned lane_b = obase;
        float* const tp = gp + (int64_t)bd.slot * slot_elems;
        const int64_t row_e = (int64_t)(ntx * ntz) * 256;                   // tile elements of one block row
        int64_t out_e = wave_e;                                             // ... before the tile column being stored
        int U = 0;
        auto out_step = [&](int g, auto u_tag) __attribute__((always_inline)) {
            const int zb = U < u_lo ? ZE0 + U * ZL1 : (U <= u_hi ? 0 : ZE0 + (u_lo + U - hi0) * ZL1);
            obase = lane_b + (unsigned)U * (16u * plane_b);
            edge_step(g, u_tag, integral_constant<int, 2>{}, zb);
            const bool wrap = U + 1 == ntz;
            U = wrap ? 0 : U + 1;
            out_e += wrap ? row_e : 0;
            rp = __builtin_amdgcn_make_buffer_rsrc(tp + out_e, 0, (int)live_b, 0x00020000);
            rp2 = __builtin_amdgcn_make_buffer_rsrc(tp + out_e + (int64_t)ntz * 256, 0, has2 ? (int)live_b : 0, 0x00020000);
        };
        edge_step(0, integral_constant<int, 0>{}, integral_constant<int, 1>{}, 0);
        int g = 1;
#pragma unroll 1
        for (; g + PF <= ntl + LA; g += PF) {
            out_step(g, integral_constant<int, 1>{});
            out_step(g + 1, integral_constant<int, 0>{});
        }
        if (g < ntl + LA) out_step(g, integral_constant<int, 1>{});
        return;
    } else if constexpr (EDGE) {
        using std::integral_constant;
        static_assert(PF == 2, "the head and tail of the LDS form are written for a ring of two");
        if constexpr (LA == 1) {
            edge_step(0, integral_constant<int, 0>{}, integral_constant<int, 1>{}, 0);
            edge_step(1, integral_constant<int, 1>{}, integral_constant<int, 2>{}, ZE0);
        } else {
            edge_step(0, integral_constant<int, 0>{}, integral_constant<int, 1>{}, 0);
            edge_step(1, integral_constant<int, 1>{}, integral_constant<int, 1>{}, 0);
            edge_step(2, integral_constant<int, 0>{}, integral_constant<int, 2>{}, ZE0);
            edge_step(3, integral_constant<int, 1>{}, integral_constant<int, 2>{}, ZE0 + ZL1);
        }
    } else {
#pragma unroll 1
        for (int t0 = 0; t0 < tA; t0 += PF) {
#pragma unroll
            for (int u = 0; u < PF; ++u)
                if (t0 + u < t_end) step(t0 + u, std::false_type{}, std::integral_constant<int, -1>{}, raw[u], outP[u], outQ[u], std::integral_constant<int, 0>{}, 0);
        }
    }
    if (nB > 0) {
        // interior Z fragments (the generic steps may have left an edge set in the registers)
        if (!ZLDS && zset != u_lo) {
            zset = u_lo;
#pragma unroll
            for (int ks = 0; ks < NKZ; ++ks)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    zw[ks][k][0] = zt[((size_t)(u_lo * NKZ + ks) * 2 + k) * 128];
                    zw[ks][k][1] = zt[((size_t)(u_lo * NKZ + ks) * 2 + k) * 128 + 64];
                }
        }
        // nothing may be pending at the loop head: a wait for the fragment loads above, placed inside the loop
        // at their first use, would be a static vmcnt(N) that in steady state waits for the previous step's stores
        // (LDS form: no fragment loads, and the head's steps have left what a turn of the loop leaves)
        if constexpr (!EDGE) __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0)
        // (rotating form: step j of a turn writes slot NT - 1 + j (mod NT): the generic steps leave tile t in slot NT - 2;
        //  SPLIT: slot j, the generic steps leave z tiles t - 3 .. t in slots 0 .. 3)
        auto turn = [&](int t0, auto... J) __attribute__((always_inline)) {
            (step(t0 + decltype(J)::value, std::true_type{},
                  std::integral_constant<int, ROT ? ((SPLIT ? 0 : NT - 1) + decltype(J)::value) % NT : -1>{},
                  raw[decltype(J)::value % PF], outP[decltype(J)::value % PF], outQ[decltype(J)::value % PF],
                  std::integral_constant<int, 0>{}, 0), ...);
        };
        if constexpr (!ROT) {
#pragma unroll 1
            for (int t0 = tA; t0 < tB; t0 += PF) {
#pragma unroll
                for (int u = 0; u < PF; ++u) step(t0 + u, std::true_type{}, std::integral_constant<int, -1>{}, raw[u], outP[u], outQ[u], std::integral_constant<int, 0>{}, 0);
            }
        } else {
#pragma unroll 1
            for (int t0 = tA; t0 < tB; t0 += GROUP) {
                using std::integral_constant;
                turn(t0, integral_constant<int, 0>{}, integral_constant<int, 1>{}, integral_constant<int, 2>{}, integral_constant<int, 3>{});
                static_assert(GROUP == 4, "a turn is four steps in every class");
            }
        }
    }
    if constexpr (EDGE) {
        // tail: whole rings, then the odd step; output tile U = t - LA >= u_lo reads the interior table while
        // U <= u_hi (the steps a whole turn or ring had no room for) and its own slot after that
        using std::integral_constant;
        auto zb_of = [&](int U) __attribute__((always_inline)) { return U <= u_hi ? 0 : ZE0 + (u_lo + U - hi0) * ZL1; };
        int t0 = tB;
#pragma unroll 1
        for (; t0 + PF <= t_end; t0 += PF) {
            edge_step(t0, integral_constant<int, 0>{}, integral_constant<int, 2>{}, zb_of(t0 - LA));
            edge_step(t0 + 1, integral_constant<int, 1>{}, integral_constant<int, 2>{}, zb_of(t0 + 1 - LA));
        }
        if (t0 < t_end) edge_step(t0, integral_constant<int, 0>{}, integral_constant<int, 2>{}, zb_of(t0 - LA));
        return;
    }
#pragma unroll 1
    for (int t0 = tB; t0 < t_end; t0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u)
            if (t0 + u < t_end) step(t0 + u, std::false_type{}, std::integral_constant<int, -1>{}, raw[u], outP[u], outQ[u], std::integral_constant<int, 0>{}, 0);
    }
