// kdf_binned_slabsort.inc -- kernel A of the binned pipeline.  kdf_binned.h includes this text twice: once as it always
// was (kb_slabsort_kernel<KW, SLICED>), once with KB_SLAB_GATED defined (kb_slabsort_gated_kernel<KW>), the form that counts
// behind an armed prefilter (kdf_prefilter.h): admit[tile] holds the tile's admitted windows, written by the gate kernel,
// and is ANDed into the thread's validity bits as soon as they are formed -- one more load per tile, prefetched with the
// stream.  Two expansions of one text rather than one body behind two wrappers: kernel A sits at the register limit, and
// its plain and SLICED forms must come out of the compiler exactly as they did before the gated form existed.
#ifdef KB_SLAB_GATED
template <int KW>
__global__ __launch_bounds__(KB_A_THREADS) void kb_slabsort_gated_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid, uint64_t n_tiles, uint64_t n_end, int k,
    KbPlan plan, KbScratch s, uint32_t slabs_per_wg, const uint64_t *__restrict__ admit)
{
    constexpr bool SLICED = false;                                      // (a prefilter and key_parts are refused together)
#else
template <int KW, bool SLICED>
__global__ __launch_bounds__(KB_A_THREADS) void kb_slabsort_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid, uint64_t n_tiles, uint64_t n_end, int k,
    KbPlan plan, KbScratch s, uint32_t slabs_per_wg)
{
#endif
    constexpr int WPT = KbCfg<KW>::WPT, TPT = 64 / WPT, SLAB = KbCfg<KW>::SLAB, NT = KB_A_THREADS;
    constexpr uint32_t TILES_PER_SLAB = NT / TPT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t *slo = (uint64_t *)smem;                                   // [SLAB + 64]: [SLAB + lane] = the lane's trash slot
    KbEnt2 *s2 = (KbEnt2 *)smem;                                        // wide: the image holds (h, hi) pairs
    // Invalid windows (N, read ends: 22 % of the window slots of 150 bp reads) are ranked like the others, branch-free, on
    // DUMMY counters -- ONE PER LANE: with a single dummy counter a quarter of a wave's lanes hit the same LDS word in every
    // rank instruction and the same trash slot in every scatter (SQ_LDS_ADDR_CONFLICT: 318 M of the kernel's 831 M active
    // LDS cycles, profiles/r03b_lds_counters.txt).
    uint32_t *hist = (uint32_t *)(smem + (size_t)(SLAB + 64) * 8 * KW); // [bins + 1 ..]: [DUMMY + lane] = counters of invalid windows (never read)
    uint32_t *offs = hist + (1 << KB_C1_MAX) + 96;                      // [bins + 1 ..]: offs[DUMMY + lane] = SLAB + lane, the lane's trash slot
    constexpr int DUMMY = (1 << KB_C1_MAX) + 1;             // (index 2^c1 <= 1024 holds the slab's total)
    const int nb = 1 << plan.c1;
    for (int i = threadIdx.x; i <= DUMMY; i += NT) hist[i] = 0;
    if (threadIdx.x < 64) offs[DUMMY + threadIdx.x] = (uint32_t)SLAB + threadIdx.x;
    __syncthreads();
    const uint64_t slab0 = (uint64_t)blockIdx.x * slabs_per_wg;
    if (slab0 * TILES_PER_SLAB >= n_tiles) return;                     // uniform
    KbWindows<KW> win;
    win.load(packed, invalid, slab0 * TILES_PER_SLAB + threadIdx.x / TPT, n_tiles, n_end, threadIdx.x % TPT, k);
#ifdef KB_SLAB_GATED
    win.valid &= (uint32_t)(admit[min(slab0 * TILES_PER_SLAB + threadIdx.x / TPT, n_tiles - 1)] >> win.p0_);
#endif
    KB_T_INIT;
    for (uint32_t sl = 0; sl < slabs_per_wg; ++sl) {
        const uint64_t slab = slab0 + sl;
        if (slab * TILES_PER_SLAB >= n_tiles) break;                  // uniform
        // (the thread index is made opaque once per slab, as in KbPipe::iter: the compiler would otherwise keep the per-lane
        // addresses of the whole loop body in registers of their own across the loop -- and spill: this kernel has 128)
        uint32_t tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        KB_T(s.trash, 18);                                               // (loop turn-around: B4, win = nxt)
        KbWindows<KW> nxt;
#ifdef KB_SLAB_GATED
        // the next slab's admitted windows travel with its prefetched words (out-of-range threads read the last tile, as issue() does)
        const uint64_t adm_nxt = admit[min((slab + 1) * TILES_PER_SLAB + tid / TPT, n_tiles - 1)];
#endif
        {
            // prefetch of the next slab's words: loads only; (tile >= n_tiles handles "no next slab")
            const bool more = sl + 1 < slabs_per_wg;
            nxt.issue(packed, invalid, more ? (slab + 1) * TILES_PER_SLAB + tid / TPT : n_tiles,
                      n_tiles, n_end, tid % TPT, k);
        }
        // Branch-free ranking: invalid windows (~4 %) go to a dummy counter
        // hist[DUMMY], so the WPT returning LDS atomics issue back to back with
        // ONE wait instead of WPT serialized round trips inside exec branches.
        uint64_t klo[WPT], khi[KW == 2 ? WPT : 1];
        uint32_t br[WPT];                       // bin << 16 | rank  (rank < SLAB <= 16384)
#pragma unroll
        for (int u = 0; u < WPT; ++u) {
            uint64_t hsh, hi; win.stored(u, hsh, hi);
            klo[u] = hsh; if constexpr (KW == 2) khi[u] = hi;
            const bool ok = ((win.valid >> u) & 1) && (!SLICED || kdf_slice(hsh, plan.key_parts) == plan.key_part);
            const uint32_t bin = ok ? kb_coarse(plan, hsh) : (uint32_t)DUMMY + (tid & 63u);
            br[u] = bin << 16;
        }
        if (KB_ABL(plan, 1024)) {                                          // (ablation: counts without ranks -- WRONG results, timing only)
#pragma unroll
            for (int u = 0; u < WPT; ++u) atomicAdd(&hist[br[u] >> 16], 1u);
        } else {
#pragma unroll
        for (int u = 0; u < WPT; ++u) br[u] |= atomicAdd(&hist[br[u] >> 16], 1u) & 0xFFFFu;
        }
        KB_T(s.trash, 10);                                               // keys, bins, rank atomics issued
        kb_lds_barrier();                                               // B1: all ranks taken
        KB_T(s.trash, 11);                                               // ... ranks back, barrier
#if KB_A_SCAN == 0
        // exclusive scan of hist[0..nb) by one wave: each lane owns a contiguous strip, read and written 16 bytes at a
        // time; offs[nb] = the slab's valid windows (kdf_scan.h)
        if (tid < 64) kb_strip_exscan(hist, offs, nb, tid);
#else
        // exclusive scan of hist[0..nb): wave w owns the bins [64 w, 64 w + 64); what lies below them is summed by the
        // wave itself (lane l adds hist[l + 64 j], j < w: independent reads, one wave reduction) -- no extra barrier, and
        // no wave walks 16 dependent LDS round trips while fifteen wait (the one-wave scan: ~0.5 us per slab)
        if ((int)tid < ((nb + 63) & ~63)) {                     // whole waves
            const int w = tid >> 6, l = tid & 63;
            uint32_t below = 0;
            for (int j = 0; j < w; ++j) below += hist[l + 64 * j];      // (w is wave-uniform)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o);
            const uint32_t v = (int)tid < nb ? hist[tid] : 0u;
            uint32_t inc = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { uint32_t t = __shfl_up(inc, o); if (l >= o) inc += t; }
            if ((int)tid < nb) offs[tid] = below + inc - v;
            if ((int)tid == nb - 1) offs[nb] = below + inc;   // the slab's valid windows
        }
#endif
        KB_T(s.trash, 12);                                               // scan (wave 0)
        kb_lds_barrier();                                               // B2: offsets ready
        KB_T(s.trash, 13);
        {
            // invalid windows land on their lane's trash slot (offs[DUMMY + lane] = SLAB + lane, rank masked off)
            uint32_t pos[WPT];
#pragma unroll
            for (int u = 0; u < WPT; ++u) {
                const uint32_t bin = br[u] >> 16;
                pos[u] = offs[bin] + ((bin >= (uint32_t)DUMMY) ? 0u : (br[u] & 0xFFFF));
            }
#pragma unroll
            for (int u = 0; u < WPT; ++u) {
                if constexpr (KW == 2) s2[pos[u]] = KbEnt2{klo[u], khi[u]};
                else slo[pos[u]] = klo[u];
            }
        }
        // the slab's offset row (coalesced) while the image settles; the histogram is zeroed for the next slab
        {
            uint16_t *orow = s.off + slab * (uint64_t)(nb + 1);
            // (straight-line: nb + 1 <= NT + 1 words -- the last one of nb = NT goes with thread 0; as a loop the compiler
            // unrolled it eight times, with 28 address registers)
            if ((int)tid <= nb) { orow[tid] = (uint16_t)offs[tid]; hist[tid] = 0; }
            if (nb == NT && tid == 0) { orow[NT] = (uint16_t)offs[NT]; hist[NT] = 0; }
            // (the dummy counters are never read: they may run on)
        }
        // (Measured and dropped, round 3: the NEXT slab's keys computed here, between scatter and B3, with its words
        // requested before the write-out -- 3.93 against 3.15 ms at k = 31, 6.95 against 5.61 at k = 63: the key arithmetic at
        // the top of the loop is what the previous slab's 128 KB of stores drain under.)
        // retire the prefetched words of the next slab BEFORE the write-out is issued:
        // vmcnt retires in order, so a later wait for these loads would also wait
        // for every store issued in between
        KB_T(s.trash, 14);                                               // scatter + offset row
        nxt.finish();
#ifdef KB_SLAB_GATED
        nxt.valid &= (uint32_t)(adm_nxt >> nxt.p0_);
#endif
        asm volatile("" :: "v"(nxt.e[0]), "v"(nxt.e[1]), "v"(nxt.valid));
        KB_T(s.trash, 15);                                               // next slab's words retired
        kb_lds_barrier();                                               // B3: sorted image complete
        KB_T(s.trash, 16);
        {
            // ONE contiguous block per slab: 16 bytes per lane and step
            // (Measured and dropped: all eight ds_read_b128 of a lane first, pinned in registers, then its stores -- no
            // spill, but 2.541 / 2.535 against 2.544 / 2.510 ms at k = 31 and 4.31 against 4.23 at k = 63, DESIGN.md 3.2: sixteen
            // waves already cover one another's LDS round trips here.)
            // Streaming stores (KB_A_NT): the block is read once, by the piece sort, after the whole stream has gone through
            // the caches -- the step 10.81 -> 10.77 ms, every run below every run without the hint.  (The same hint on the
            // piece sort's write-out: 4.04 -> 4.51 ms for that kernel; on the dump's dense stores: within the noise.)
            const uint32_t nv = KB_ABL(plan, 256) ? 0u : offs[nb];          // (ablation 256: no write-out -- timing only)
            if constexpr (KW == 2) {
                KbEnt2 *dst = (KbEnt2 *)s.tmp + slab * (uint64_t)SLAB;
                for (uint32_t i = tid; i < nv; i += NT) kb_store_once16(&dst[i], &s2[i]);
            } else {
                ulonglong2 *dst = (ulonglong2 *)(s.tmp + slab * (uint64_t)SLAB);
                const ulonglong2 *src = (const ulonglong2 *)slo;
                for (uint32_t i = tid; i < (nv + 1) / 2; i += NT) kb_store_once16(&dst[i], &src[i]);      // (SLAB is even: the odd tail stays inside the slab's block)
            }
        }
        KB_T(s.trash, 17);                                               // write-out issued
#ifdef KB_TIMING
        if (tid == 0) atomicAdd((unsigned long long *)&s.trash[8 + 19], 1ull);
#endif
#if KB_A_B4
        kb_lds_barrier();                                               // B4: image free (stores still draining)
#endif
        win = nxt;
    }
}
