// crh_scan_body.hpp -- the body of k_scan and k_scan_list (crh_kernels.hpp), included INSIDE each of the two kernels with
// CRH_SCAN_LIST defined 0 / 1.  One text, two kernels: with CRH_SCAN_LIST 0 it is k_scan's body word for word, so that
// kernel's code does not depend on the list variant existing (tools/isa_diff.py compares the two builds); with 1, item i is
// tile tilelist[i * tile_stride] instead of tile i * tile_stride.  Not a header: it has no meaning outside those braces.
//
// CRH_SCAN_CLASSES 0 / 1 (k_scan_cls, k_scan_list_cls: a batch whose queries carry different filters).  With 0 the text is
// the one above, token for token after preprocessing.  With 1 every lane tests the rows of a tile against the validity word of
// ITS query's filter class: the tile's 8 class words (classmask[tile], interleaved so that they are one 32-byte scalar load)
// are fetched where the plain kernels fetch rowmask[tile] -- their OR is that union word -- and after the MFMAs each lane
// picks word cls0 (column block 0) / cls1 (block 1) with a v_cndmask tree.  The picked word stands where vmask stands in the
// MODE 0 maxima and the MODE 1 pass test; the wave-uniform early-out keeps the union word.  No vector load is added to the
// tile loop: the ring's vmcnt count holds.
    static_assert(KSTEPS % RING == 0, "ring must divide the k-steps of a tile");
    __shared__ u32x4 qs[QB * KSTEPS * 64];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;

    // (Preparing the queries HERE, in the seed scan -- every workgroup building the image in its own LDS, workgroup 0 writing it
    // out for the later kernels -- was built and measured in round 3: it removes k_prep_queries' launch and adds the same time to
    // this kernel, 119.7 us against 119.3 us around the main scan.  Not shipped.)
    for (int i = tid; i < QB * KSTEPS * 64; i += WAVES * 64) qs[i] = qfrag[i];
    float t0 = 0.f, t1 = 0.f;
    if (MODE == 1) {
        t0 = tau[lane & 31];
        t1 = QB == 2 ? tau[32 + (lane & 31)] : INFINITY;
    }
#if CRH_SCAN_CLASSES
    // the class of the lane's query in each column block: 4 bits per query, 8 queries per word of the kernel argument
    // (padding columns of a short batch are class 0; their tau is +inf)
    const int cq = lane & 31;
    const uint32_t cw0 = cq < 8 ? qclass.w[0] : cq < 16 ? qclass.w[1] : cq < 24 ? qclass.w[2] : qclass.w[3];
    const uint32_t cw1 = cq < 8 ? qclass.w[4] : cq < 16 ? qclass.w[5] : cq < 24 ? qclass.w[6] : qclass.w[7];
    const uint32_t cls0 = (cw0 >> ((cq & 7) * 4)) & 7u;
    const uint32_t cls1 = QB == 2 ? (cw1 >> ((cq & 7) * 4)) & 7u : 0u;
#endif
    __syncthreads();

    const int total = gridDim.x * WAVES;
    const int gw = blockIdx.x * WAVES + wave;
    u32x4 *mylist = wave_lists + (size_t)gw * wave_cap;
    unsigned int wcnt = 0;

    int i = gw;
    const int lslot = lane_slot(lane);   // (the lane's 16 bytes inside a piece)
#if CRH_SCAN_LIST
    // item -> tile through the list: i is wave-uniform, so the entry is a scalar load; the entry of the wave's NEXT tile is
    // fetched at the top of the current tile, a whole tile before the run-ahead loads need it
    int64_t tcur = i < nitems ? (int64_t)tilelist[(int64_t)i * tile_stride] : 0;
    const u32x4 *xp = xt + (size_t)tcur * (KSTEPS * 64) + lslot;
#else
    const u32x4 *xp = xt + (size_t)(i < nitems ? (int64_t)i * tile_stride : 0) * (KSTEPS * 64) + lslot;
#endif
    u32x4 ring[RING];
    if (i < nitems) {
#pragma unroll
        for (int d = 0; d < RING; ++d) nt_load(ring[d], xp + piece_off(d));
    }
    while (i < nitems) {
        const int inext = i + total;
#if CRH_SCAN_LIST
        const int64_t tile = tcur;
        const int64_t tnext = (inext < nitems) ? (int64_t)tilelist[(int64_t)inext * tile_stride] : tcur;
        const u32x4 *xn = (inext < nitems) ? xt + (size_t)tnext * (KSTEPS * 64) + lslot : xp;
#else
        const int64_t tile = (int64_t)i * tile_stride;
        const u32x4 *xn = (inext < nitems) ? xt + (size_t)((int64_t)inext * tile_stride) * (KSTEPS * 64) + lslot : xp;
#endif
#if CRH_SCAN_CLASSES
        const u32x8 cwords = classmask[tile];  // wave-uniform, 32 bytes aligned -> ONE scalar load of the tile's 8 class words
#else
        const uint32_t vmask = rowmask[tile];  // wave-uniform -> scalar load
#endif
        // the query image is loop-invariant: without this the compiler hoists all 96 LDS pieces (384 VGPRs)
        // out of the tile loop and spills; the clobber makes it re-read qs per tile, as intended
        asm volatile("" ::: "memory");

        f32x16 a0 = {0}, a1 = {0};
        u32x4 b0 = qs[lane], b1 = qs[(QB - 1) * KSTEPS * 64 + lane];
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            // order pinned by the sched_barrier: next step's query pieces (LDS), this step's two MFMAs, then the
            // load that refills this ring slot RING steps ahead (it may belong to the wave's next tile).
            const int s1 = (s + 1 < KSTEPS) ? s + 1 : s;
            const u32x4 nb0 = qs[s1 * 64 + lane];
            const u32x4 nb1 = qs[((QB - 1) * KSTEPS + s1) * 64 + lane];
            nt_wait<RING - 1>(ring[s % RING]);   // the oldest of the RING loads in flight has landed (issue order)
            const bf16x8 xa = __builtin_bit_cast(bf16x8, ring[s % RING]);
            if (MODE == 2) {   // read-ceiling probe: the loads alone, kept alive by an empty asm
                asm volatile("" ::"v"(ring[s % RING]));
            } else {
                a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa, __builtin_bit_cast(bf16x8, b0), a0, 0, 0, 0);
                if (QB == 2) a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa, __builtin_bit_cast(bf16x8, b1), a1, 0, 0, 0);
            }
            const int sp = s + RING;
            const u32x4 *src = (sp < KSTEPS) ? xp + piece_off(sp) : xn + piece_off(sp - KSTEPS);
            nt_load(ring[s % RING], src);
            b0 = nb0;
            b1 = nb1;
            __builtin_amdgcn_sched_barrier(0);
        }

#if CRH_SCAN_CLASSES
        // the union word (what rowmask holds for the tile-list kernels): seven scalar ORs instead of a second load
        const uint32_t vmask = cwords[0] | cwords[1] | cwords[2] | cwords[3] | cwords[4] | cwords[5] | cwords[6] | cwords[7];
        const uint32_t vm0 = class_pick(cwords, cls0);
        const uint32_t vm1 = QB == 2 ? class_pick(cwords, cls1) : 0u;
#else
        const uint32_t vm0 = vmask, vm1 = vmask;
#endif
        if (MODE == 2) {
            // nothing: the probe measures what the same access pattern reads with no arithmetic and no candidate logic
        } else if (MODE == 0) {
            float m0 = -INFINITY, m1 = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const bool ok0 = (vm0 >> row) & 1u, ok1 = (vm1 >> row) & 1u;
                m0 = fmaxf(m0, ok0 ? a0[r] : -INFINITY);
                m1 = fmaxf(m1, ok1 ? a1[r] : -INFINITY);
            }
            m0 = fmaxf(m0, __shfl_xor(m0, 32));
            m1 = fmaxf(m1, __shfl_xor(m1, 32));
            if (h == 0) {
                gmax[(size_t)i * 64 + lane] = m0;
                if (QB == 2) gmax[(size_t)i * 64 + 32 + lane] = m1;
            }
        } else {
            float m0 = a0[0], m1 = a1[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) {
                m0 = fmaxf(m0, a0[r]);
                m1 = fmaxf(m1, a1[r]);
            }
            const bool any = (m0 >= t0) || (m1 >= t1);
            if (__ballot(any) != 0ull && vmask != 0u) {
                const uint32_t rowbase = (uint32_t)(tile * 32);
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) {
                    const float tq = qb ? t1 : t0;
                    const uint32_t vq = qb ? vm1 : vm0;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                        const float sc = qb ? a1[r] : a0[r];
                        const bool pass = ((vq >> row) & 1u) && (sc >= tq);
                        const unsigned long long pm = __ballot(pass);
                        if (pm != 0ull) {
                            const unsigned int pre = __builtin_amdgcn_mbcnt_hi(
                                (unsigned int)(pm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)pm, 0u));
                            const unsigned int pos = wcnt + pre;
                            if (pass && pos < (unsigned int)wave_cap) {
                                u32x4 e;
                                e.x = f32_bits(sc);
                                e.y = rowbase + row;
                                e.z = (uint32_t)(qb * 32 + (lane & 31));
                                e.w = 0u;
                                mylist[pos] = e;
                            }
                            wcnt += (unsigned int)__popcll(pm);
                        }
                    }
                }
            }
        }
        xp = xn;
        i = inext;
#if CRH_SCAN_LIST
        tcur = tnext;
#endif
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the run-ahead loads of the last tile are still in flight

    if (MODE == 1) {
        // Hand the workgroup's candidates over to the per-query lists: count per query in LDS, reserve
        // one contiguous range per (workgroup, query) with 64 global atomics, scatter.
        __syncthreads();  // every wave is done with qs (and its list stores have completed)
        unsigned int *wc = reinterpret_cast<unsigned int *>(qs);  // [WAVES] counts, [64] hist, [64] base, [64] off
        unsigned int *hist = wc + WAVES;
        unsigned int *base = hist + 64;
        unsigned int *off = base + 64;
        if (lane == 0) {
            wc[wave] = wcnt < (unsigned int)wave_cap ? wcnt : (unsigned int)wave_cap;
            atomicMax(&status->max_wave_cnt, wcnt);
            if (wcnt > (unsigned int)wave_cap) atomicAdd(&status->wave_overflow, 1u);
        }
        if (tid < 64) {
            hist[tid] = 0u;
            off[tid] = 0u;
        }
        __syncthreads();
        const u32x4 *wl = wave_lists + (size_t)blockIdx.x * WAVES * wave_cap;
        for (int w = 0; w < WAVES; ++w) {
            const unsigned int n = wc[w];
            for (unsigned int e = tid; e < n; e += WAVES * 64) atomicAdd(&hist[wl[(size_t)w * wave_cap + e].z & 63u], 1u);
        }
        __syncthreads();
        if (tid < 64) base[tid] = hist[tid] ? atomicAdd(&qcount[tid], hist[tid]) : 0u;
        __syncthreads();
        for (int w = 0; w < WAVES; ++w) {
            const unsigned int n = wc[w];
            for (unsigned int e = tid; e < n; e += WAVES * 64) {
                const u32x4 c = wl[(size_t)w * wave_cap + e];
                const unsigned int q = c.z & 63u;
                const unsigned int idx = base[q] + atomicAdd(&off[q], 1u);
                if (idx < (unsigned int)qcap) {
                    u32x2 o;
                    o.x = c.x;
                    o.y = c.y;
                    qlist[(size_t)q * qcap + idx] = o;
                }
            }
        }
    }
