// The part of k_jacobi_band (stencil.hip) that follows the choice of the cell form: the sweeps, the hand-offs of the persistent form, the
// store of p and the gradient epilogue.  Not a translation unit: the kernel includes this text where `constexpr bool FUSED` says which
// cell a sweep takes -- once at function scope in the instantiations that have the exact cell only (they then compile to the instructions
// they had before there were two forms; as a lambda body they do not), and inside a lambda instantiated per form in those that have both.
// No include guard: the kernel includes it twice on purpose.
    if constexpr (FUSED) {
#pragma unroll
        for (int k = 0; k < RPW; ++k)
#pragma unroll
            for (int c = 0; c < VEC; ++c) dv[k][c] = jacobi_cell_nd(dv[k][c]);
    }
    // one row of a sweep src -> dst; up / dn: the rows above and below (registers, or the neighbour wave's edge row)
    auto row = [&](const float (&src)[RPW][VEC], float (&dst)[RPW][VEC], int k, const float (&up)[VEC], const float (&dn)[VEC]) {
        const float lin = wave_shr1(src[k][VEC - 1]), rin = wave_shl1(src[k][0]);
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            const float l = c > 0 ? src[k][c - 1] : lin;
            const float r = c < VEC - 1 ? src[k][c + 1] : rin;
            if constexpr (FUSED) dst[k][c] = jacobi_cell_fused(up[c], dn[c], l, r, dv[k][c]);
            else dst[k][c] = jacobi_cell_exact(up[c], dn[c], l, r, dv[k][c]);
        }
        dst[k][0] = first_col ? 0.f : dst[k][0];              // column ring: only the two edge cells need a select
        dst[k][VEC - 1] = last_col ? 0.f : dst[k][VEC - 1];
    };
    // a wave's first and last row go to edge buffer `par`; the neighbour waves' facing rows come back from it (after a barrier)
    auto publish = [&](const float (&r)[RPW][VEC], int par) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            edge[par][wave][0][j0 + c] = r[0][c];
            edge[par][wave][1][j0 + c] = r[RPW - 1][c];
        }
    };
    float above[VEC], below[VEC];
    auto fetch = [&](int par) {
        const float *eu = &edge[par][wave > 0 ? wave - 1 : 0][1][j0];            // top wave: value unused (ring or halo row)
        const float *ed = &edge[par][wave < JB_NW - 1 ? wave + 1 : JB_NW - 1][0][j0];
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            above[c] = eu[c];
            below[c] = ed[c];
        }
    };
    // the two rows that need `above` / `below`, with the row ring (grid row 0 / H-1: 2 waves of a grid) as wave-uniform selects -- as
    // scalar branches they cost more in register copies at the control-flow merges (16 v_mov per sweep) than the 2 * VEC v_cndmask
    // they save
    auto edge_rows = [&](const float (&src)[RPW][VEC], float (&dst)[RPW][VEC]) {
        row(src, dst, 0, above, src[1]);
        row(src, dst, RPW - 1, src[RPW - 2], below);
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            dst[0][c] = ring_k == 0 ? 0.f : dst[0][c];
            dst[RPW - 1][c] = ring_k == RPW - 1 ? 0.f : dst[RPW - 1][c];
        }
    };
    // One sweep src -> dst (register ping-pong: no row copies); par selects the LDS edge buffer.  The order is software-pipelined over two
    // sweeps (PIPE): `above` / `below` of src are already in registers when a sweep starts (run() primes them); the wave first computes the
    // two rows that need them and publishes those rows of dst -- the NEXT sweep's edge rows -- into the other buffer, covers the stores with
    // NA interior rows, passes the barrier, issues the reads of the next sweep's `above` / `below`, and covers those with the remaining
    // interior rows: no wave waits on an LDS trip with nothing to issue.  What a sweep then costs is the vector issue of its rows, which the
    // four waves of a SIMD take in turns, the youngest last, the others waiting for it at the barrier (stamps: DESIGN 3.1, profiles/r07).
    // Buffer s & 1 is rewritten in sweep s + 2, after barrier s + 1, which every wave passes only after it has consumed (in sweep
    // s + 1's first two rows) what it read from buffer s.  RPW 2 / 3 have 0 / 1 interior rows: the same chain as the plain order.
    // Plain order (PIPE false): publish src's edge rows, interior rows, barrier, read, the two edge rows.
    // STAIRS (jb_prio_stairs): the wave's issue priority falls stage by stage from one barrier to the next -- 3, 2 behind the barrier, 1 over
    // the edge rows and the publish, 0 ahead of the barrier -- so a wave that is behind outranks the ones ahead of it instead of waiting
    // for its turn by age; no instruction of a stage moves (profiles/r34).
    constexpr bool PIPE = jb_pipelined(VEC, RPW, PERSIST);
    constexpr bool STAIRS = jb_prio_stairs(VEC, RPW, PERSIST, FOLD);   // the wave's priority falls from one barrier to the next (jacobi_plan.h)
    constexpr int NA = jb_rows_before_barrier(RPW, STAIRS);   // interior rows ahead of the barrier (cover the stores); the rest follow the reads
    static_assert(!STAIRS || (PIPE && RPW - 2 > NA), "the staircase needs the pipelined order and an interior row behind the barrier");
    auto sweep = [&](const float (&src)[RPW][VEC], float (&dst)[RPW][VEC], int par) {
        if constexpr (PIPE) {
            wave_prio<STAIRS, 1>();                           // the next sweep's edge rows and their publish
            edge_rows(src, dst);
            publish(dst, par);
            __builtin_amdgcn_sched_barrier(0);                // first: the neighbours' next sweep waits on these stores
            wave_prio<STAIRS, 0>();                           // the rows ahead of the barrier: whoever is still behind goes first
#pragma unroll
            for (int k = 1; k < 1 + NA; ++k) row(src, dst, k, src[k - 1], src[k + 1]);
            __builtin_amdgcn_sched_barrier(0);                // (hipcc otherwise sinks these rows below the barrier)
            __syncthreads();
            wave_prio<STAIRS, 3>();                           // the reads and the first interior rows behind the barrier
            fetch(par);
            __builtin_amdgcn_sched_barrier(0);                // reads in flight before the rows that cover them
#pragma unroll
            for (int k = 1 + NA; k < RPW - 1; ++k) {
                if (k == RPW - 2) wave_prio<STAIRS, 2>();     // the last of them
                row(src, dst, k, src[k - 1], src[k + 1]);
            }
            __builtin_amdgcn_sched_barrier(0);                // (the wait for the reads belongs to the next sweep's first rows)
        } else {
            publish(src, par);
            __builtin_amdgcn_sched_barrier(0);                // publish first: the neighbours' edge rows wait on these stores
#pragma unroll
            for (int k = 1; k < RPW - 1; ++k) row(src, dst, k, src[k - 1], src[k + 1]);
            __builtin_amdgcn_sched_barrier(0);                // (hipcc otherwise sinks these rows below the barrier)
            __syncthreads();
            fetch(par);
            edge_rows(src, dst);
        }
    };
    float pw[RPW][VEC];
    auto run = [&](int n) {                                   // n sweeps, result in pv
        if constexpr (PIPE) {
            // prime the pipeline: pv's own edge rows (after a hand-off: with the halo rows just reloaded) through buffer 1, which the
            // first sweep leaves alone.  Every caller has a workgroup barrier between a run's last reads and this store.
            publish(pv, 1);
            __syncthreads();
            fetch(1);
        }
        int it = 0;
        for (; it + 2 <= n; it += 2) {
            sweep(pv, pw, 0);
            sweep(pw, pv, 1);
        }
        if (it < n) {
            sweep(pv, pw, 0);
#pragma unroll
            for (int k = 0; k < RPW; ++k)
#pragma unroll
                for (int c = 0; c < VEC; ++c) pv[k][c] = pw[k][c];
        }
        wave_prio<STAIRS, 0>();                               // outside a sweep a wave runs at priority 0
    };
    if constexpr (!PERSIST) {
        run(iters);
    } else {
        const int me = b * nb + band;
        const unsigned row_off = (unsigned)(base * sizeof(float));          // byte offset of this lane's cells of tile row row0 in x0 / x1
        const unsigned pitch_b = (unsigned)(g.pc * sizeof(float));
        const unsigned xbytes = (unsigned)((size_t)(sy.grid0 + sy.ngrids) * g.sc * sizeof(float));
        const __amdgpu_buffer_rsrc_t rx0 = __builtin_amdgcn_make_buffer_rsrc(sy.x0, 0, xbytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rx1 = __builtin_amdgcn_make_buffer_rsrc(sy.x1, 0, xbytes, 0x00020000);
        int done = 0;
        if (threadIdx.x == 0) handoff_failed = 0;             // (read only after a hand-off: at least two workgroup barriers later)
        for (int c = 0; c < sy.chunks; ++c) {
            const int n = jb_run_sweeps(iters, done, sy.chunks, c);
            run(n);
            done += n;
            if (c == sy.chunks - 1) break;
            const __amdgpu_buffer_rsrc_t rx = (c & 1) ? rx1 : rx0;
            // publish: the `halo` owned rows next to each inner boundary
#pragma unroll
            for (int k = 0; k < RPW; ++k) {
                const int gi = row0 + k;
                const bool pub = (band > 0 && gi >= own0 && gi < own0 + halo) || (band < nb - 1 && gi >= own1 - halo && gi < own1);
                if (pub) stv_sc1<VEC>(rx, row_off + k * pitch_b, pv[k]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its stores before the barrier
            __syncthreads();
            if (threadIdx.x == 0) {
                const unsigned tgt = sy.base + (unsigned)c + 1u;
                if (!(sy.fault && me == sy.grid0 * nb))       // (fault injection for the time-out test: one band never publishes)
                    __hip_atomic_store(sy.flags + me, tgt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const long long t0 = wall_clock64();
                for (;;) {
                    const bool up = band == 0 ||
                        (int)(__hip_atomic_load(sy.flags + me - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - tgt) >= 0;
                    const bool dn = band == nb - 1 ||
                        (int)(__hip_atomic_load(sy.flags + me + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - tgt) >= 0;
                    if (up && dn) break;
                    if (__hip_atomic_load(sy.flags + sy.abort_slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                        handoff_failed = 1;                   // another band gave up: this band's halo rows are stale too
                        break;
                    }
                    if (wall_clock64() - t0 > sy.timeout_ticks) {
                        __hip_atomic_store(sy.flags + sy.abort_slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(sy.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        handoff_failed = 1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
            }
            __syncthreads();
            // refresh: the halo rows (the neighbours' published rows; rows of the tile beyond them stay stale, which `halo` sweeps
            // cannot carry into the owned range)
#pragma unroll
            for (int k = 0; k < RPW; ++k) {
                const int gi = row0 + k;
                const bool need = (gi >= own0 - halo && gi < own0) || (gi >= own1 && gi < own1 + halo);
                if (need) ldv_sc1<VEC>(pv[k], rx, row_off + k * pitch_b);
            }
        }
        // A hand-off that did not complete leaves stale halo rows, and p, u, v are updated in place: results that cannot be right must not
        // look like data.  The band's p becomes NaN (so do its u, v through the gradient below, and every frame of the grid from here on);
        // the host reads *status at its next synchronising call (smk_sim_status) and reports the time-out for THIS projection.
        if (sy.chunks > 1 && handoff_failed) {
#pragma unroll
            for (int k = 0; k < RPW; ++k)
#pragma unroll
                for (int c = 0; c < VEC; ++c) pv[k][c] = __builtin_nanf("");
        }
    }
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int gi = row0 + k;
        if (gi >= own0 && gi < own1) {
#pragma unroll
            for (int c = 0; c < VEC; ++c) p_out[base + (size_t)k * g.pc + c] = pv[k][c];
        }
    }
    if (MODE & 2) {
        // u[i,:] -= dt*(p[i,:] - p[i-1,:]) for 1 <= i <= H-1;  v[:,j] -= dt*(p[:,j] - p[:,j-1]) for 1 <= j <= W-1
        __syncthreads();                                      // all reads of the last sweep's edges are done
#pragma unroll
        for (int c = 0; c < VEC; ++c) edge[0][wave][1][j0 + c] = pv[RPW - 1][c];
        __syncthreads();
        float above[VEC];
#pragma unroll
        for (int c = 0; c < VEC; ++c) above[c] = edge[0][wave > 0 ? wave - 1 : 0][1][j0 + c];
        float *ub = u + b * g.su + (size_t)row0 * g.pc + j0, *vb = v + b * g.sv + (size_t)row0 * g.pv + j0;
#pragma unroll
        for (int k = 0; k < RPW; ++k) {
            const int gi = row0 + k;
            const float lin = wave_shr1(pv[k][VEC - 1]);
            if (gi >= own0 && gi < own1) {
                // whole-row read-modify-write (VEC cells per lane as one load / one store; the untouched cells -- row 0 of u, column 0
                // of v -- are written back unchanged)
                float un[VEC], vn[VEC];
                const int ku = KEEP ? keep_of(gi, 1) : -1, kv = KEEP ? keep_of(gi, 0) : -1;
                // (without KEEP the slots are the constant -1 and these reads dead: clang's bounds check still sees the index)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Warray-bounds"
                if (ku >= 0) ldv<VEC>(un, &keep[ku][j0]);
                else ldv<VEC>(un, ub + (size_t)k * g.pc);
                if (kv >= 0) ldv<VEC>(vn, &keep[kv][j0]);
                else ldv<VEC>(vn, vb + (size_t)k * g.pv);
#pragma clang diagnostic pop
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    if (gi >= 1) {                            // gi == row0 == 0 only in the first wave of band 0: skipped
                        const float pu = k > 0 ? pv[k - 1][c] : above[c];
                        const float gr = pv[k][c] - pu;
                        un[c] = un[c] - g.dt * gr;
                    }
                    const float pl = c > 0 ? pv[k][c - 1] : lin;
                    const float gr = pv[k][c] - pl;
                    const float nv = vn[c] - g.dt * gr;
                    vn[c] = (c == 0 && first_col) ? vn[c] : nv;   // j >= 1 (j <= W-1 always holds here)
                }
                if (gi >= 1) stv<VEC>(ub + (size_t)k * g.pc, un);
                stv<VEC>(vb + (size_t)k * g.pv, vn);
            }
        }
    }
