// The k-mer index of `hinge seed` and `hinge overlap` (include/hinge_hip.h, "hinge index"; DESIGN.md 3.12).  Included by hinge_capi.hip.
// Host work here: the choice of the path (where / HINGE_INDEX_DEVICE / the scratch budget), the two running sums of the range's
// lengths, the launches of index_kernels.h and the recursion of its scan, the check of the two counts that come back.  The host
// path is seed_build_index (seed_index.h) and the uploads, as before.
#include <chrono>

struct IndexState {
    DevBuf eoff, ping, pong, table, sums, scal;    // the device build's scratch, reused from range to range
    DevBuf codes, gpos, off;                       // hinge_index_build's result (hinge_index_fetch)
    int64_t n_kept = 0;
    int32_t n_seqs = -1;                           // of the last hinge_index_build (-1: none)
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // hinge_index_last_stats
};

static long long seed_env(const char* name, long long def);

static void index_release(hinge_ctx* ctx) {
    IndexState* t = ctx->idx_st;
    if (!t) return;
    DevBuf* all[] = {&t->eoff, &t->ping, &t->pong, &t->table, &t->sums, &t->scal, &t->codes, &t->gpos, &t->off};
    for (DevBuf* b : all) release(*b);
    delete t;
    ctx->idx_st = nullptr;
}

static IndexState* index_state(hinge_ctx* ctx) {
    if (!ctx->idx_st) ctx->idx_st = new IndexState();
    return ctx->idx_st;
}

static void index_stats_reset(hinge_ctx* ctx) {
    for (int64_t& v : index_state(ctx)->stats) v = 0;
}

// elements of the scan's totals below `len` elements, all levels
static long long index_scan_sums_elems(long long len) {
    long long tot = 0;
    while (len > IDX_SCAN_CHUNK) { len = idx_chunks(len); tot += len; }
    return tot;
}

// the device build's scratch for n entries of n_seqs sequences
static long long index_scratch_bytes(long long n, long long n_seqs) {
    const long long table = (long long)IDX_DIGITS * idx_tiles(n);
    return 16 * n + 4 * table + 4 * index_scan_sums_elems(std::max(table, n + 1)) + 8 * (n_seqs + 1) + 16;
}

// a[0 .. len) becomes its exclusive scan; sums: index_scan_sums_elems(len) elements
static int index_scan(hinge_ctx* ctx, unsigned* a, long long len, unsigned* sums) {
    const long long nb = idx_chunks(len);
    if (nb > 1) {
        { ProfScope _ps(ctx, KID_INDEX_SCAN);
          hipLaunchKernelGGL(k_index_scan_sums, dim3((unsigned)nb), dim3(64), IDX_LDS_BYTES, ctx->stream, (const unsigned*)a, len, sums); }
        CK(hipGetLastError());
        int rc;
        if ((rc = index_scan(ctx, sums, nb, sums + nb))) return rc;
    }
    { ProfScope _ps(ctx, KID_INDEX_SCAN);
      hipLaunchKernelGGL(k_index_scan_apply, dim3((unsigned)std::max(nb, 1ll)), dim3(64), IDX_LDS_BYTES, ctx->stream, a, len, nb > 1 ? (const unsigned*)sums : (const unsigned*)nullptr); }
    CK(hipGetLastError());
    return HINGE_OK;
}

// The entries of the range on the device, from the resident bases of DB 0: kept ones into codes / gpos, the two counts back.
// d_off: the range's off[] on the device (index_build uploads it on both paths).
static int index_build_device(hinge_ctx* ctx, int first, int nr, int k, int max_occ, const long long* d_off, const std::vector<long long>& h_eoff, DevBuf& codes, DevBuf& gpos,
                              int64_t* n_kept, int64_t* dropped) {
    IndexState* t = ctx->idx_st;
    CnsState* s = ctx->cns;
    const long long n = h_eoff[(size_t)nr];
    int rc;
    *n_kept = 0; *dropped = 0;
    if ((rc = ensure(ctx, codes, sizeof(uint32_t) * 1)) || (rc = ensure(ctx, gpos, sizeof(int32_t) * 1))) return rc;
    t->stats[5] = idx_passes(k);
    if (n == 0) return HINGE_OK;
    const long long n_tiles = idx_tiles(n), table_len = (long long)IDX_DIGITS * n_tiles;
    if ((rc = ensure(ctx, t->eoff, sizeof(long long) * ((size_t)nr + 1)))) return rc;
    if ((rc = ensure(ctx, t->ping, sizeof(unsigned long long) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, t->pong, sizeof(unsigned long long) * (size_t)n))) return rc;       // (>= the n + 1 flags of the filter)
    if ((rc = ensure(ctx, t->table, sizeof(unsigned) * (size_t)table_len))) return rc;
    if ((rc = ensure(ctx, t->sums, sizeof(unsigned) * (size_t)std::max(index_scan_sums_elems(std::max(table_len, n + 1)), 1ll)))) return rc;
    if ((rc = ensure(ctx, t->scal, 16))) return rc;
    t->stats[7] = std::max(t->stats[7], (int64_t)index_scratch_bytes(n, nr));
    CK(hipMemcpyAsync(t->eoff.p, h_eoff.data(), sizeof(long long) * ((size_t)nr + 1), hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemsetAsync(t->ping.p, 0xff, sizeof(unsigned long long) * (size_t)n, ctx->stream));   // poison: what a kernel did not write sorts last and breaks the counts
    CK(hipMemsetAsync(t->pong.p, 0xff, sizeof(unsigned long long) * (size_t)n, ctx->stream));
    CK(hipMemsetAsync(t->scal.p, 0, 16, ctx->stream));
    CnsSeqs SB{(const unsigned char*)s->bps[0].p, (const long long*)s->boff[0].p, (const int*)s->rlen[0].p};
    int seq_top = 0, occ_top = 0;
    for (long long v = 1; v <= (long long)nr; v <<= 1) seq_top = (int)v;       // the searches' trip counts: fixed here
    for (int v = 1; v <= max_occ; v <<= 1) occ_top = v;
    const unsigned g64 = (unsigned)((n + 63) / 64);
    unsigned long long* src = (unsigned long long*)t->ping.p;
    unsigned long long* dst = (unsigned long long*)t->pong.p;
    {
        ProfScope _ps(ctx, KID_INDEX_EXTRACT);
        hipLaunchKernelGGL(k_index_extract, dim3(g64), dim3(64), 0, ctx->stream, SB, first, nr, seq_top, k, d_off, (const long long*)t->eoff.p, (int)n, src);
    }
    CK(hipGetLastError());
    for (int pass = 0; pass < idx_passes(k); pass++) {
        const int shift = 32 + 8 * pass;
        {
            ProfScope _ps(ctx, KID_INDEX_HIST);
            hipLaunchKernelGGL(k_index_hist, dim3((unsigned)n_tiles), dim3(64), IDX_LDS_BYTES, ctx->stream, (const unsigned long long*)src, (int)n, shift, n_tiles, (unsigned*)t->table.p);
        }
        CK(hipGetLastError());
        if ((rc = index_scan(ctx, (unsigned*)t->table.p, table_len, (unsigned*)t->sums.p))) return rc;
        {
            ProfScope _ps(ctx, KID_INDEX_SCATTER);
            hipLaunchKernelGGL(k_index_scatter, dim3((unsigned)n_tiles), dim3(64), IDX_LDS_BYTES, ctx->stream, (const unsigned long long*)src, dst, (int)n, shift, n_tiles,
                               (const unsigned*)t->table.p);
        }
        CK(hipGetLastError());
        std::swap(src, dst);
    }
    // ---- the filter: src holds the sorted pairs, dst is free and takes the n + 1 flags ------------------------------------------------------------------------
    unsigned* flags = (unsigned*)dst;
    CK(hipMemsetAsync(flags, 0xff, sizeof(unsigned) * ((size_t)n + 1), ctx->stream));
    {
        ProfScope _ps(ctx, KID_INDEX_FLAG);
        hipLaunchKernelGGL(k_index_flag, dim3((unsigned)((n + 1 + 63) / 64)), dim3(64), 0, ctx->stream, (const unsigned long long*)src, (int)n, max_occ, occ_top, flags, (unsigned*)t->scal.p);
    }
    CK(hipGetLastError());
    if ((rc = index_scan(ctx, flags, n + 1, (unsigned*)t->sums.p))) return rc;
    unsigned h_cnt[2] = {0xffffffffu, 0xffffffffu};                           // kept, dropped
    CK(hipMemcpyAsync(&h_cnt[0], flags + n, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(&h_cnt[1], t->scal.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    const long long kept = h_cnt[0], drop = h_cnt[1];
    if (kept > n || kept + drop * ((long long)max_occ + 1) > n) return fail(ctx, HINGE_E_DEVICE, "index build: the counts of the device build do not fit the entries (a slot was never written)");
    if ((rc = ensure(ctx, codes, sizeof(uint32_t) * (size_t)std::max(kept, 1ll)))) return rc;
    if ((rc = ensure(ctx, gpos, sizeof(int32_t) * (size_t)std::max(kept, 1ll)))) return rc;
    if (kept) {
        CK(hipMemsetAsync(codes.p, 0xff, sizeof(uint32_t) * (size_t)kept, ctx->stream));
        CK(hipMemsetAsync(gpos.p, 0xff, sizeof(int32_t) * (size_t)kept, ctx->stream));
        {
            ProfScope _ps(ctx, KID_INDEX_COMPACT);
            hipLaunchKernelGGL(k_index_compact, dim3(g64), dim3(64), 0, ctx->stream, (const unsigned long long*)src, (const unsigned*)flags, (int)n, (unsigned)kept, (unsigned*)codes.p,
                               (int*)gpos.p);
        }
        CK(hipGetLastError());
        CK(hipStreamSynchronize(ctx->stream));
    }
    *n_kept = kept; *dropped = drop;
    return HINGE_OK;
}

// The index of sequences [first, first + nr) of DB 0 into codes / gpos / off (device) and h_off (host): the caller has checked
// the range, k, max_occ and that the range holds fewer than 2^31 bases.  where: 1 device, 0 host, -1 HINGE_INDEX_DEVICE (default 1);
// a device build whose scratch would exceed HINGE_INDEX_SCRATCH_MB (2048; HINGE_INDEX_SCRATCH_BYTES) is a host build.
static int index_build(hinge_ctx* ctx, int first, int nr, int k, int max_occ, int where, DevBuf& codes, DevBuf& gpos, DevBuf& off, std::vector<long long>& h_off, int64_t* n_kept,
                       int64_t* dropped) {
    const auto t0 = std::chrono::steady_clock::now();
    IndexState* t = index_state(ctx);
    CnsState* s = ctx->cns;
    std::vector<long long> h_eoff((size_t)nr + 1, 0);
    h_off.assign((size_t)nr + 1, 0);
    for (int c = 0; c < nr; c++) {
        const long long len = s->h_rlen[0][(size_t)(first + c)];
        h_off[(size_t)c + 1] = h_off[(size_t)c] + len;
        h_eoff[(size_t)c + 1] = h_eoff[(size_t)c] + std::max(len - k + 1, 0ll);
    }
    const long long n = h_eoff[(size_t)nr];
    int rc;
    if ((rc = ensure(ctx, off, sizeof(long long) * ((size_t)nr + 1)))) return rc;
    CK(hipMemcpyAsync(off.p, h_off.data(), sizeof(long long) * ((size_t)nr + 1), hipMemcpyHostToDevice, ctx->stream));
    if (where < 0) where = seed_env("HINGE_INDEX_DEVICE", 1) != 0;
    long long budget = std::max(1ll, seed_env("HINGE_INDEX_SCRATCH_MB", 2048)) << 20;
    budget = std::max(1ll, seed_env("HINGE_INDEX_SCRATCH_BYTES", budget));
    const bool device = where != 0 && index_scratch_bytes(n, nr) <= budget;
    if (device) {
        if ((rc = index_build_device(ctx, first, nr, k, max_occ, (const long long*)off.p, h_eoff, codes, gpos, n_kept, dropped))) return rc;
        t->stats[3]++;
    } else {
        SeedIndex ix;
        seed_build_index(s->h_bps0.data(), s->h_boff0.data() + first, s->h_rlen[0].data() + first, nr, k, max_occ, ix);
        const size_t ne = ix.codes.size();
        if ((rc = ensure(ctx, codes, sizeof(uint32_t) * std::max<size_t>(ne, 1)))) return rc;
        if ((rc = ensure(ctx, gpos, sizeof(int32_t) * std::max<size_t>(ne, 1)))) return rc;
        if (ne) {
            CK(hipMemcpyAsync(codes.p, ix.codes.data(), sizeof(uint32_t) * ne, hipMemcpyHostToDevice, ctx->stream));
            CK(hipMemcpyAsync(gpos.p, ix.gpos.data(), sizeof(int32_t) * ne, hipMemcpyHostToDevice, ctx->stream));
        }
        *n_kept = (int64_t)ne; *dropped = ix.dropped_codes;
        t->stats[4]++;
    }
    CK(hipStreamSynchronize(ctx->stream));
    t->stats[0] += n;
    t->stats[1] += *n_kept;
    t->stats[2] += *dropped;
    t->stats[6] += (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return HINGE_OK;
}

extern "C" {

int hinge_index_tile(void) { return IDX_TILE; }

int hinge_index_build(hinge_ctx* ctx, int32_t first, int32_t n_seqs, int32_t k, int32_t max_occ, int32_t where, int64_t* n_entries, int64_t* dropped_codes) {
    if (!ctx || !ctx->cns || !n_entries || !dropped_codes || where < -1 || where > 1) return fail(ctx, HINGE_E_ARG, "hinge_index_build: bad arguments (call hinge_consensus_set_db first)");
    if (k < SEED_K_MIN || k > SEED_K_MAX || max_occ < 1 || max_occ > SEED_OCC_MAX) return fail(ctx, HINGE_E_ARG, "hinge_index_build: k 8..16, max_occ 1..256");
    CnsState* s = ctx->cns;
    if (first < 0 || n_seqs < 0 || (long long)first + n_seqs > s->n_seq[0]) return fail(ctx, HINGE_E_RANGE, "hinge_index_build: sequences outside DB 0");
    long long total = 0;
    for (int c = 0; c < n_seqs; c++) total += s->h_rlen[0][(size_t)(first + c)];
    if (total >= (1ll << 31)) return fail(ctx, HINGE_E_CAPACITY, "hinge_index_build: a range of 2^31 or more bases");
    CK(hipSetDevice(ctx->device));
    IndexState* t = index_state(ctx);
    index_stats_reset(ctx);
    t->n_seqs = -1;
    std::vector<long long> h_off;
    int rc;
    if ((rc = index_build(ctx, first, n_seqs, k, max_occ, where, t->codes, t->gpos, t->off, h_off, &t->n_kept, dropped_codes))) return rc;
    t->n_seqs = n_seqs;
    *n_entries = t->n_kept;
    return HINGE_OK;
}

int hinge_index_fetch(hinge_ctx* ctx, int64_t cap, uint32_t* codes, int32_t* gpos, int64_t* off) {
    if (!ctx || !ctx->idx_st || ctx->idx_st->n_seqs < 0 || cap < 0 || !off || (ctx->idx_st->n_kept > 0 && (!codes || !gpos))) return fail(ctx, HINGE_E_ARG, "hinge_index_fetch: no hinge_index_build yet, or bad arguments");
    IndexState* t = ctx->idx_st;
    if (t->n_kept > cap) return fail(ctx, HINGE_E_CAPACITY, "hinge_index_fetch: the output arrays must hold what hinge_index_build counted");
    CK(hipSetDevice(ctx->device));
    static_assert(sizeof(long long) == sizeof(int64_t), "off is copied as it is");
    if (t->n_kept) {
        CK(hipMemcpyAsync(codes, t->codes.p, sizeof(uint32_t) * (size_t)t->n_kept, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(gpos, t->gpos.p, sizeof(int32_t) * (size_t)t->n_kept, hipMemcpyDeviceToHost, ctx->stream));
    }
    CK(hipMemcpyAsync(off, t->off.p, sizeof(int64_t) * ((size_t)t->n_seqs + 1), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return HINGE_OK;
}

int hinge_index_last_stats(hinge_ctx* ctx, int64_t* out) {
    if (!ctx || !ctx->idx_st || !out) return fail(ctx, HINGE_E_ARG, "hinge_index_last_stats: no index was built yet");
    for (int k = 0; k < 8; k++) out[k] = ctx->idx_st->stats[k];
    return HINGE_OK;
}

}  // extern "C"
