// fixup_kernel's body (tmh_engine.hip), included once per kernel: by fixup_kernel<SITES, SER, IVL> with
// DEM = false and by fixup_demand_kernel<SITES> with SER, IVL and DEM all true.  (Text, not a
// function: the kernels that existed before the demand registers compile exactly as they did.)
    constexpr bool REG = SER && IVL;
    constexpr int RC = DEM ? TMH_DEMAND_COLS : TMH_REGISTERS_COLS;
    TraceView tr{};
    SeriesView se{};
    IntervalsView ivv{};
    if constexpr (SER && !IVL) se = ov;
    else if constexpr (IVL) ivv = ov;
    else tr = ov;
    const uint32_t nrec = min(*sg.nfix, sg.fixcap);
    const int ne = (int)min(*n_events, ev_cap_dev(nsteps));
    const uint32_t lane = threadIdx.x;   // one wave per workgroup
    for (uint32_t r0 = blockIdx.x * FIX_RPW; r0 < nrec; r0 += gridDim.x * FIX_RPW) {   // wave-uniform
        const uint32_t rw = r0 + (lane >> 2);
        uint32_t word = 0;
        if (rw < nrec) {
            const uint4 m = sg.fix[rw].mask;
            const uint32_t w = lane & 3;
            word = w == 0 ? m.x : (w == 1 ? m.y : (w == 2 ? m.z : m.w));
        }
        uint32_t cum = __popc(word);   // inclusive prefix sum over the wave's words
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(cum, d, 64);
            if (lane >= (uint32_t)d) cum += u;
        }
        const uint32_t total = __builtin_amdgcn_readfirstlane(__shfl(cum, 63, 64));
        for (uint32_t k0 = 0; k0 < total; k0 += 64) {   // wave-uniform
            const uint32_t k = k0 + lane;
            // the word holding flagged second k: the first q with cum[q] > k (every lane
            // takes part in the shuffles; lanes past the total search for nothing)
            uint32_t lo = 0;
#pragma unroll
            for (uint32_t h = 32; h; h >>= 1)
                if (__shfl(cum, (int)(lo + h - 1), 64) <= k) lo += h;
            const uint32_t wq = __shfl(word, (int)lo, 64);
            const uint32_t cq = __shfl(cum, (int)lo, 64);
            if (k >= total) continue;
            uint32_t m = wq;
            for (uint32_t rank = k - (cq - __popc(wq)); rank; --rank) m &= m - 1;   // drop the lower set bits
            const uint32_t i = (lo & 3) * 32 + (uint32_t)(__ffs(m) - 1);   // second of the record's block
            const FixRec& fr = sg.fix[r0 + (lo >> 2)];
            const uint32_t c = fr.c;
            if (c >= n || fr.b >= sg.nblk) continue;   // (never appended: the expansion records live chains only)
            const BlockDesc db = desc[fr.b];
            const uint32_t j = fr.b * BLOCK_STEPS + i;
            const uint32_t cw = (lo & 3) == 0 ? fr.cov.x : ((lo & 3) == 1 ? fr.cov.y : ((lo & 3) == 2 ? fr.cov.z : fr.cov.w));
            const bool covered = (cw >> (i & 31)) & 1u;
            float pv32, meter, pv;
            if (!redo_second<SITES>(kp, dp, st, sg, n, c, chain0, W0, utc0, j, db, covered, SER || IVL || sv.acc != nullptr, events, ne,
                                    tab64, tab32, sun, pv32, meter, pv))
                continue;
            const float res = meter - pv, res32 = meter - pv32;   // second_body's residual
            const size_t o = (size_t)j * tr.ld + c;
            if (tr.pv) reinterpret_cast<float*>(tr.pv)[o] = pv;
            if (tr.residual) reinterpret_cast<float*>(tr.residual)[o] = res;
            if constexpr (SER && !IVL) {
                const long long dq = (long long)series_q<float>(pv) - (long long)series_q<float>(pv32);
                const uint32_t g = se.group_chains ? c / se.group_chains : 0u;
                if (dq) atomicAdd(se.sum + (size_t)g * se.gstride + (size_t)j * 4, (unsigned long long)dq);
            }
            if constexpr (IVL) {
                const long long dq = (long long)series_q<float>(pv) - (long long)series_q<float>(pv32);
                const uint32_t k = (ivv.rel0 + j) / ivv.interval_s;
                if constexpr (!REG) {
                    if (dq) atomicAdd(ivv.sum + (size_t)k * 4 * ivv.ld + gid(kp.ids, c), (unsigned long long)dq);
                } else {
                    const int qm = series_q<float>(meter);
                    const long long dex = (long long)max(series_q<float>(pv) - qm, 0) - (long long)max(series_q<float>(pv32) - qm, 0);
                    unsigned long long* cell = ivv.sum + (size_t)k * RC * ivv.ld + gid(kp.ids, c);
                    if (dq) atomicAdd(cell, (unsigned long long)dq);
                    if (dex - dq) atomicAdd(cell + 4 * ivv.ld, (unsigned long long)(dex - dq));
                    if (dex) atomicAdd(cell + 5 * ivv.ld, (unsigned long long)dex);
                    if constexpr (DEM) {
                        const int d = qm - series_q<float>(pv);
                        const uint32_t o = ivv.rel0 + j - k * ivv.interval_s;
                        __hip_atomic_fetch_max(cell + 6 * ivv.ld, demand_key((uint32_t)max(d, 0), o), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_fetch_max(cell + 7 * ivv.ld, demand_key((uint32_t)max(-d, 0), o), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
            if (sv.acc) {
                atomicAdd(&sg.corr[c], (double)pv - (double)pv32);
                atomicAdd(&sg.corr[(size_t)n + c], (double)res - (double)res32);
                __hip_atomic_fetch_max(sg.acc_mx + c, max_key((double)res), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (sv.hist) {
                atomicAdd((unsigned long long*)&sv.hist[hist_bin_rt<float>(sv, res)], 1ull);
            }
        }
    }
