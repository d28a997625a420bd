// fm_part_launch.inc -- part of fm_kernels.hip (one translation unit; included there, in this order: helpers, decimate, audio, cascade, chan, launch).
// the one-row audio kernel of the drop-in and every extern "C" launcher
// ------------------------------------------------------------------ launchers

#define LAUNCH_RET() return (int)hipGetLastError()

/* magic for n / d (truncating, by sign and magnitude) as a multiply-high: floor(a / d) == (a * (2^32 / d + 1)) >> 32 for 0 <= a <= amax whenever
 * amax * d < 2^32 (the error of the constant, < 1 / 2^32 per unit of a, stays under 1 / d); 0 = use the plain division */
static unsigned dc_div_magic(int d, long long amax)
{
	if (d < 2 || amax * (long long)d >= (1ll << 32))
		return 0u;
	return (unsigned)((1ull << 32) / (unsigned)d + 1);
}

// rx_power's boxcar with the sums of every wave's stored outputs left in wave_sums[span * 4 + wave] = {I, Q} (k_fm_decimate<.., DCS>): prescaled input,
// no rotation, phase 0
extern "C" int rxk_pw_boxcar_sums(void *stream, const int16_t *iq, u64 T, int ds, uint32_t *lp_raw, uint32_t *head, uint32_t *tail, int *wave_sums)
{
	const unsigned grid = (unsigned)((T + RXK_DEC_SPAN - 1) / RXK_DEC_SPAN);
	const unsigned magic = (unsigned)((1ull << 32) / (unsigned)ds + 1);
	const unsigned magic24 = ((u64)(RXK_DEC_SPAN + 4 + ds) * (u64)ds < (1ull << 24)) ? (1u << 24) / (unsigned)ds + 1 : 0u;
	const unsigned slot_cap = (RXK_DEC_SPAN + ds) / ds + 4 + 64;
	const size_t shm = (size_t)(slot_cap + 4) * sizeof(uint32_t);
	if (magic24)
		hipLaunchKernelGGL((k_fm_decimate<true, false, false, true, false, true>), dim3(grid), dim3(DEC_THREADS), shm, (hipStream_t)stream, (const u32x4 *)iq, T, ds, 0,
		                   magic, magic24, lp_raw, head, tail, slot_cap, 0, (int16_t *)nullptr, 0, (int2 *)wave_sums);
	else
		hipLaunchKernelGGL((k_fm_decimate<true, false, false, false, false, true>), dim3(grid), dim3(DEC_THREADS), shm, (hipStream_t)stream, (const u32x4 *)iq, T, ds, 0,
		                   magic, magic24, lp_raw, head, tail, slot_cap, 0, (int16_t *)nullptr, 0, (int2 *)wave_sums);
	LAUNCH_RET();
}

// the raw capture with -E rdc's block averages subtracted on the way (k_fm_decimate<.., RDC>): blocks of spans_per_block whole spans, rdc_avg = two ints per block
extern "C" int rxk_fm_decimate_rdc(void *stream, const int16_t *iq, u64 T, int ds, int p0, int rotate, uint32_t *lp_raw, uint32_t *head, uint32_t *tail,
                                   int lp_sparse, int16_t *pcm, int pcm_chl2, const int *rdc_avg, unsigned spans_per_block)
{
	if (!pcm || ds > RXK_LP_SPARSE_MAX_DS)
		lp_sparse = 0;
	const unsigned grid = (unsigned)((T + RXK_DEC_SPAN - 1) / RXK_DEC_SPAN);
	const unsigned magic = (unsigned)((1ull << 32) / (unsigned)ds + 1);
	const unsigned magic24 = ((u64)(RXK_DEC_SPAN + 4 + ds) * (u64)ds < (1ull << 24)) ? (1u << 24) / (unsigned)ds + 1 : 0u;
	const unsigned slot_cap = (RXK_DEC_SPAN + ds) / ds + 4 + 64;
	const size_t shm = (size_t)(slot_cap + 4) * sizeof(uint32_t);          /* 4-byte slots, the unbiased scan: a sample minus its dc average can reach 256 */
	hipStream_t s = (hipStream_t)stream;
	const u32x4 *p = (const u32x4 *)iq;
#define GO3(RT, DC, D24) hipLaunchKernelGGL((k_fm_decimate<false, RT, DC, D24, false, false, true>), dim3(grid), dim3(DEC_THREADS), shm, s, p, T, ds, p0, \
		magic, magic24, lp_raw, head, tail, slot_cap, lp_sparse, pcm, pcm_chl2, (int2 *)nullptr, rdc_avg, spans_per_block)
#define GO(RT) do { \
		if (pcm) { if (magic24) GO3(RT, true, true); else GO3(RT, true, false); } \
		else { if (magic24) GO3(RT, false, true); else GO3(RT, false, false); } } while (0)
	if (rotate) GO(true); else GO(false);
#undef GO
#undef GO3
	LAUNCH_RET();
}

extern "C" int rxk_fm_decimate(void *stream, const int16_t *iq, u64 T, int ds, int p0, int prescaled, int rotate,
                               uint32_t *lp_raw, uint32_t *head, uint32_t *tail, int lp_sparse, int16_t *pcm, int pcm_chl2)
{
	if (!pcm || ds > RXK_LP_SPARSE_MAX_DS)
		lp_sparse = 0;
	const unsigned grid = (unsigned)((T + RXK_DEC_SPAN - 1) / RXK_DEC_SPAN);
	const unsigned magic = (unsigned)((1ull << 32) / (unsigned)ds + 1);
	/* floor(q / ds) = (q << 8) * magic24 >> 32 is exact while q * ds < 2^24; q <= span + 4 + ds */
	const unsigned magic24 = ((u64)(RXK_DEC_SPAN + 4 + ds) * (u64)ds < (1ull << 24)) ? (1u << 24) / (unsigned)ds + 1 : 0u;
	const unsigned slot_cap = (RXK_DEC_SPAN + ds) / ds + 4 + 64;      /* + one turn of lanes past the last output (read, never used) */
	/* 16-byte slot records (the prefix selection left to the reader, dec_prefix_wide) where they stay small: raw input, ds >= 64
	 * (at most 5 KiB of LDS per workgroup); prescaled input and ds < 64 keep the 4-byte slots */
	const bool wide = !prescaled && ds >= 64;
	const size_t shm = (size_t)((wide ? 4 : 1) * slot_cap + 4) * sizeof(uint32_t);
	hipStream_t s = (hipStream_t)stream;
	const u32x4 *p = (const u32x4 *)iq;
#define GO4(PS, RT, DC, D24, W) hipLaunchKernelGGL((k_fm_decimate<PS, RT, DC, D24, W>), dim3(grid), dim3(DEC_THREADS), shm, s, p, T, ds, p0, \
		magic, magic24, lp_raw, head, tail, slot_cap, lp_sparse, pcm, pcm_chl2)
#define GO3(PS, RT, DC, D24) do { if (!PS && wide) GO4(PS, RT, DC, D24, !PS); else GO4(PS, RT, DC, D24, false); } while (0)
#define GO(PS, RT) do { \
		if (pcm) { if (magic24) GO3(PS, RT, true, true); else GO3(PS, RT, true, false); } \
		else { if (magic24) GO3(PS, RT, false, true); else GO3(PS, RT, false, false); } } while (0)
	if (prescaled) GO(true, false);
	else if (rotate) GO(false, true);
	else GO(false, false);
#undef GO
#undef GO3
#undef GO4
	LAUNCH_RET();
}

// k_fm_decimate_lane takes ds = 4 .. 12 and the even ds up to 32 (NP <= 16 vectors per lane; an odd ds needs W = 4 windows per lane, 4 ds registers
// of raw samples: those stay with k_fm_decimate_small).  A/B in one process, pipelined 4 GiB steps (profiles/r06_ab_dec_lane.txt): level with
// k_fm_decimate_small at ds = 5 / 6, +1..5 % at 4 / 7 / 8 / 9, +13..37 % at 10 / 11 / 12 (where the LDS-staged kernel has no unrolled window sum).
// That A/B was taken at commit 509b7aa against the unrolled k_fm_decimate_small<., 4..8, .> instances, which this kernel then replaced.
// $RXGPU_DL_TW: tiles a wave walks (default 4; the tests walk 1..5).  A workgroup asks for 52000 bytes of LDS -- three per CU: the occupancy cap
// that leaves wave slots to the audio stages of the run before (A/B: 40000 / 52000 / 65536 within 1 %, no cap 4-10 % slower).
#ifdef RXK_NO_LANE                                             /* scratch builds only: A/B against k_fm_decimate_small (tools: $RXGPU_LIB_FLAVOUR) */
static bool dl_takes(int ds) { (void)ds; return false; }
#else
static bool dl_takes(int ds) { return ds >= 4 && (ds <= 12 || (ds <= 32 && !(ds & 1))); }
#endif

template <bool RT, int DS>
static void dl_launch(hipStream_t s, const uint32_t *iq, u64 T, int p0, u64 M, int16_t *pcm, int pcm_chl2)
{
	constexpr int W = dl_geom<DS>::W, NP = dl_geom<DS>::NP, NS = dl_geom<DS>::NS;
	static_assert((size_t)4 * NS * 64 * NP * 16 <= 65536, "the ring of a workgroup fits the default dynamic LDS limit");
	const char *e = rxgpu_knob("RXGPU_DL_TW");
	const unsigned tw = e && atoi(e) >= 1 && atoi(e) <= 4096 ? (unsigned)atoi(e) : 4u;
	// a tile starts at sample L G - p0 + RP = 4 (NP G - c), c = (p0 - RP) / 4: on a 128-byte line iff NP G == c (mod 8).  Odd NP: one lane
	// number g_a mod 8 does it for every tile of every wave; even NP: the g_a that leaves the fewest low bits (A/B: 3.5 % of the kernel)
	const int c = (p0 - (p0 & 3)) / 4;
	int g_a = 0, best = -1;
	for (int g = 0; g < 8; g++) {
		const int d = ((NP * g - c) % 8 + 8) % 8, z = d == 0 ? 3 : __builtin_ctz((unsigned)d);
		if (z > best) { best = z; g_a = g; }
	}
	const u64 lanes = (M + W - 1) / W, per_wave = 64ull * tw - DL_HALO;
	const unsigned n_waves = lanes > (u64)g_a ? (unsigned)((lanes - (u64)g_a + per_wave - 1) / per_wave) : 1u;
	const unsigned grid = ((n_waves + 3) / 4 + 7u) & ~7u;
	size_t lds = (size_t)4 * NS * 64 * NP * 16;
	if (lds < 52000)
		lds = 52000;
#define DLK(RPV) hipLaunchKernelGGL((k_fm_decimate_lane<RT, DS, RPV>), dim3(grid), dim3(256), lds, s, iq, T, p0, M, pcm, pcm_chl2, tw, n_waves, g_a)
	switch (p0 & 3) {
	case 0: DLK(0); break;
	case 1: DLK(1); break;
	case 2: DLK(2); break;
	default: DLK(3); break;
	}
#undef DLK
}

extern "C" int rxk_fm_decimate_small(void *stream, const int16_t *iq, u64 T, int ds, int p0, int rotate, unsigned long long M, int16_t *pcm,
                                     int pcm_chl2)
{
	{
		if (dl_takes(ds) && M) {
			hipStream_t s = (hipStream_t)stream;
			const uint32_t *p = (const uint32_t *)iq;
#define DL(D) case D: if (rotate) dl_launch<true, D>(s, p, T, p0, M, pcm, pcm_chl2); else dl_launch<false, D>(s, p, T, p0, M, pcm, pcm_chl2); break
			switch (ds) { DL(4); DL(5); DL(6); DL(7); DL(8); DL(9); DL(10); DL(11); DL(12); DL(14); DL(16); DL(18); DL(20); DL(22); DL(24); DL(26); DL(28); DL(30); DL(32); }
#undef DL
			LAUNCH_RET();
		}
	}
	/* what is left for this kernel: the odd ds from 13 to 31 (k_fm_decimate_lane would hold 4 ds registers of raw samples per lane).
	 * The staged span, padded to a fifth of the CU's LDS: five workgroups per CU (20 waves) run the kernel as fast as eight do, and the audio
	 * stages of the previous run -- long, latency-bound waves on the other stream -- always find slots beside them */
	const unsigned span = dsm_span(ds);
	const unsigned grid = ((unsigned)((T + span - 1) / span) + 7u) & ~7u;
	size_t lds = (size_t)(span + 2 * DSM_HALO + 8) * 4;
	if (lds < 32000)
		lds = 32000;
	hipStream_t s = (hipStream_t)stream;
	const u32x4 *p = (const u32x4 *)iq;
	const bool four = (span + 2 * DSM_HALO) / 4 <= 1024;
#define GO(RT) do { if (four) hipLaunchKernelGGL((k_fm_decimate_small<RT, 4>), dim3(grid), dim3(256), lds, s, p, T, ds, p0, M, pcm, pcm_chl2, span, span / (unsigned)ds); \
		else hipLaunchKernelGGL((k_fm_decimate_small<RT, 5>), dim3(grid), dim3(256), lds, s, p, T, ds, p0, M, pcm, pcm_chl2, span, span / (unsigned)ds); } while (0)
	if (rotate) GO(true); else GO(false);
#undef GO
	LAUNCH_RET();
}

extern "C" int rxk_fm_decimate_generic(void *stream, const int16_t *iq, u64 T, int ds, int p0, u64 n_per_block,
                                       int prescaled, int rotate, const rxk_fm_dev *dev, uint32_t *lp, u64 M)
{
	if (!M)
		return 0;
	hipStream_t s = (hipStream_t)stream;
	if (ds >= 1 && ds <= 3 && p0 == 0 && (n_per_block & 3) == 0 && ((size_t)iq & 15) == 0) {
		/* whole windows from the run's first sample on: twelve samples per thread in three 16-byte loads (k_fm_decimate_tiny) */
		const unsigned tgrid = (unsigned)(((T + 11) / 12 + 255) / 256);
		const u32x4 *p = (const u32x4 *)iq;
#define TINY(PS, RT) do { if (ds == 1) hipLaunchKernelGGL((k_fm_decimate_tiny<PS, RT, 1>), dim3(tgrid), dim3(256), 0, s, p, T, lp, M); \
		else if (ds == 2) hipLaunchKernelGGL((k_fm_decimate_tiny<PS, RT, 2>), dim3(tgrid), dim3(256), 0, s, p, T, lp, M); \
		else hipLaunchKernelGGL((k_fm_decimate_tiny<PS, RT, 3>), dim3(tgrid), dim3(256), 0, s, p, T, lp, M); } while (0)
		if (prescaled) TINY(true, false); else if (rotate) TINY(false, true); else TINY(false, false);
#undef TINY
		LAUNCH_RET();
	}
	const unsigned grid = (unsigned)((M + 255) / 256);
	if (prescaled)
		hipLaunchKernelGGL((k_fm_decimate_generic<true>), dim3(grid), dim3(256), 0, s, (const uint32_t *)iq, T, ds, p0, n_per_block, 0, dev, lp, M);
	else
		hipLaunchKernelGGL((k_fm_decimate_generic<false>), dim3(grid), dim3(256), 0, s, (const uint32_t *)iq, T, ds, p0, n_per_block, rotate, dev, lp, M);
	LAUNCH_RET();
}

static int fm_disc_launch(void *stream, const int16_t *iq, u64 T, int ds, int p0, u64 n_per_block, int prescaled,
                          int rotate, int seams, const uint32_t *lp_raw, const uint32_t *head, const uint32_t *tail,
                          uint32_t *lp, u64 M, int first_mode, u64 uniform_k, int custom_atan, int do_tail,
                          int16_t *pcm, rxk_fm_dev *dev, rxk_flag_rec *flag_list, int *flag_cnt, int sparse, u64 n_blocks, const int *atan_lut,
                          int lp_sparse, int flag_all, int pcm_chl2, const int *rdc_avg)
{
	if (!sparse || !seams)
		lp_sparse = 0;
	/* seams == 2 (after rxk_fm_decimate_small): no span seams, just the run's first two outputs */
	const u64 n_wg = seams == 2 ? 1 : (T + RXK_DEC_SPAN - 1) / RXK_DEC_SPAN;
	/* no discriminator and no seam entries to finish (am / usb / lsb / raw, squelch behind the one-thread-per-output decimator): only the carries are left */
	const unsigned out_blocks = sparse ? (unsigned)((2 * n_wg + n_blocks + 1 + 255) / 256) : (!pcm && !seams && M) ? 1u : (unsigned)((M + 255) / 256);
	const unsigned grid = out_blocks + (do_tail ? 1 : 0);
	if (!grid)
		return 0;
	hipStream_t s = (hipStream_t)stream;
	if (prescaled)
		hipLaunchKernelGGL((k_fm_disc<true>), dim3(grid), dim3(256), 0, s, (const uint32_t *)iq, T, ds, p0, n_per_block, 0, seams,
		                   lp_raw, head, tail, lp, M, first_mode, uniform_k, custom_atan, do_tail, pcm, dev, flag_list, flag_cnt, out_blocks, sparse, n_wg, n_blocks, atan_lut, lp_sparse, flag_all, pcm_chl2, (const int *)nullptr);
	else
		hipLaunchKernelGGL((k_fm_disc<false>), dim3(grid), dim3(256), 0, s, (const uint32_t *)iq, T, ds, p0, n_per_block, rotate, seams,
		                   lp_raw, head, tail, lp, M, first_mode, uniform_k, custom_atan, do_tail, pcm, dev, flag_list, flag_cnt, out_blocks, sparse, n_wg, n_blocks, atan_lut, lp_sparse, flag_all, pcm_chl2, rdc_avg);
	LAUNCH_RET();
}

extern "C" int rxk_fm_disc(void *stream, const int16_t *iq, u64 T, int ds, int p0, u64 n_per_block, int prescaled,
                           int rotate, int seams, const uint32_t *lp_raw, const uint32_t *head, const uint32_t *tail,
                           uint32_t *lp, u64 M, int first_mode, u64 uniform_k, int custom_atan, int do_tail,
                           int16_t *pcm, rxk_fm_dev *dev, rxk_flag_rec *flag_list, int *flag_cnt, int sparse, u64 n_blocks, const int *atan_lut,
                           int lp_sparse, int flag_all, int pcm_chl2)
{
	return fm_disc_launch(stream, iq, T, ds, p0, n_per_block, prescaled, rotate, seams, lp_raw, head, tail, lp, M, first_mode, uniform_k, custom_atan, do_tail,
	                      pcm, dev, flag_list, flag_cnt, sparse, n_blocks, atan_lut, lp_sparse, flag_all, pcm_chl2, nullptr);
}

/* behind rxk_fm_decimate_rdc: the windows this kernel sums again from the raw capture take the same block averages off */
extern "C" int rxk_fm_disc_rdc(void *stream, const int16_t *iq, u64 T, int ds, int p0, u64 n_per_block, int rotate, int seams, const uint32_t *lp_raw,
                               const uint32_t *head, const uint32_t *tail, uint32_t *lp, u64 M, int custom_atan, int16_t *pcm, rxk_fm_dev *dev,
                               rxk_flag_rec *flag_list, int *flag_cnt, int sparse, u64 n_blocks, const int *atan_lut, int lp_sparse, int flag_all, int pcm_chl2,
                               const int *rdc_avg)
{
	return fm_disc_launch(stream, iq, T, ds, p0, n_per_block, 0, rotate, seams, lp_raw, head, tail, lp, M, RXK_FIRST_LOWPASS, 0, custom_atan, 1,
	                      pcm, dev, flag_list, flag_cnt, sparse, n_blocks, atan_lut, lp_sparse, flag_all, pcm_chl2, rdc_avg);
}

static unsigned magic_for(int a) { return a > 1 ? (unsigned)((1ull << 32) / (unsigned)a + 1) : 0u; }

static int bias_for(int a) { return 65536 / a + 2; }

// the 24-bit forms: the unsigned division takes (2^26/a + 1) < 2^24, i.e. a >= 5; the three-instruction step multiplies by the same
// constant with a SIGNED 24-bit multiply-high (v_mul_hi_i32_i24), so it needs 2^26/a + 1 < 2^23: a >= 9.  One predicate for both.
static bool deemph_d24(int a) { return a >= 9 && a < 256; }
static unsigned deemph_magic(int a) { return deemph_d24(a) ? (1u << 26) / (unsigned)a + 1 : magic_for(a); }
// the kernels that divide only through deemph_div / deemph_mul (k_ch_audio, k_cha_*, k_fm_row_audio) take the two-multiply 24-bit form from a = 5:
// floor(t / a) == ((t << 6) * (2^26 / a + 1)) >> 32 for every t < 2^18 whenever the constant fits 24 bits UNSIGNED (a >= 5; checked for all t and
// a = 5 .. 272).  deemph_d24 starts at 9 because the tiled rx_fm kernels' three-instruction step multiplies SIGNED 24-bit operands (de_step).
static bool deemph_d24u(int a) { return a >= 5 && a < 256; }
static unsigned deemph_magic_u(int a) { return deemph_d24u(a) ? (1u << 26) / (unsigned)a + 1 : magic_for(a); }
static int ilog2(int v) { int l = 0; while ((1 << l) < v) l++; return l; }

template <typename K>
static void deemph_lds_attr(K kernel, size_t lds)
{
	if (lds > 48 * 1024)
		(void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

extern "C" int rxk_fm_deemph_scan(void *stream, const int16_t *pcm, u64 M, int a, int group, int chunk, int warm,
                                  int lo0, int hi0, int *pre, int *p_tab, int *p_lo, int *p_gap, rxk_fm_dev *dev)
{
	if (!M)
		return 0;
	const u64 n_chunks = (M + chunk - 1) / chunk;
	const unsigned grid = (unsigned)((n_chunks + 63) / 64);
	const size_t lds = 65 * (size_t)(chunk / 8 + 1) * 16 + (size_t)(64 * group + 128) * 4;
	hipStream_t s = (hipStream_t)stream;
	const unsigned mg = deemph_magic(a);
	const int bias = bias_for(a), l2 = ilog2(chunk);
#define GO(GS, EV, D) do { deemph_lds_attr(k_fm_deemph_scan<GS, EV, D>, lds); \
		hipLaunchKernelGGL((k_fm_deemph_scan<GS, EV, D>), dim3(grid), dim3(64), lds, s, pcm, M, a, mg, bias, l2, warm, \
		                   lo0, hi0, pre, p_tab, p_lo, p_gap, dev); } while (0)
	if (group == 16) {
		if (deemph_d24(a)) { if (a & 1) GO(16, false, true); else GO(16, true, true); }
		else { if (a & 1) GO(16, false, false); else GO(16, true, false); }
	} else {
		if (a & 1) GO(64, false, true); else GO(64, true, true);
	}
#undef GO
	LAUNCH_RET();
}

extern "C" int rxk_fm_deemph_up(void *stream, u64 n_child, int group, const int *tab, const int *lo, const int *gap,
                                int *p_tab, int *p_lo, int *p_gap)
{
	const u64 parents = (n_child + DEEMPH_FAN - 1) / DEEMPH_FAN;
	const u64 threads = parents * group;
	hipLaunchKernelGGL(k_fm_deemph_up, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
	                   n_child, group, tab, lo, gap, p_tab, p_lo, p_gap);
	LAUNCH_RET();
}

extern "C" int rxk_fm_deemph_top(void *stream, int n, int group, const int *tab, const int *lo, const int *gap,
                                 int *start, rxk_fm_dev *dev)
{
	int R = 1;
	while (R * R < n) R++;
	const int nseg = (n + R - 1) / R;
	const size_t shm = ((size_t)n * group + 2 * (size_t)n + (size_t)nseg * group + nseg) * sizeof(int);
	static size_t allowed = 64 * 1024;            /* raise the dynamic-LDS cap once, not per launch */
	if (shm > allowed) {
		(void)hipFuncSetAttribute((const void *)k_fm_deemph_top, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
		allowed = 144 * 1024;
	}
	hipLaunchKernelGGL(k_fm_deemph_top, dim3(1), dim3(256), shm, (hipStream_t)stream, n, group, tab, lo, gap, start, dev);
	LAUNCH_RET();
}

extern "C" int rxk_fm_deemph_down(void *stream, u64 n_child, int group, const int *tab, const int *lo,
                                  const int *p_start, int *start)
{
	const u64 parents = (n_child + DEEMPH_FAN - 1) / DEEMPH_FAN;
	hipLaunchKernelGGL(k_fm_deemph_down, dim3((unsigned)((parents + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
	                   n_child, group, tab, lo, p_start, start);
	LAUNCH_RET();
}

extern "C" int rxk_fm_deemph_apply(void *stream, const int16_t *pcm, u64 M, int a, int group, int chunk, const int *pre,
                                   const int *p_lo, const int *p_start, int16_t *y)
{
	if (!M)
		return 0;
	const u64 n_chunks = (M + chunk - 1) / chunk;
	const unsigned grid = (unsigned)((n_chunks + 63) / 64);
	const size_t lds = 65 * (size_t)(chunk / 8 + 1) * 16;
	hipStream_t s = (hipStream_t)stream;
	const unsigned mg = deemph_magic(a);
	const int bias = bias_for(a), l2 = ilog2(chunk);
#define GO(EV, D) do { deemph_lds_attr(k_fm_deemph_apply<EV, D>, lds); \
		hipLaunchKernelGGL((k_fm_deemph_apply<EV, D>), dim3(grid), dim3(64), lds, s, pcm, M, a, mg, bias, l2, group, pre, p_lo, p_start, y); } while (0)
	if (deemph_d24(a)) { if (a & 1) GO(false, true); else GO(true, true); }
	else { if (a & 1) GO(false, false); else GO(true, false); }
#undef GO
	LAUNCH_RET();
}

extern "C" int rxk_fm_deemph_tiled_ok(int a, int group, int chunk, int fast, int slow)
{
	if (!(a & 1) || !deemph_d24(a) || (group != 16 && group != 64) || (chunk != 128 && chunk != 256))
		return 0;
	if (slow <= 0 || fast < 2 * slow || fast / slow > 32)
		return 0;
	return chunk == 128 ? 7 : 8;
}

extern "C" int rxk_fm_deemph_scan_t(void *stream, const int16_t *pcm_t, u64 M, int a, int group, int chl2, int warm, int lo0, int gap_w,
                                    void *ctab, rxk_fm_dev *dev)
{
	if (!M)
		return 0;
	const u64 n_chunks = (M + (1u << chl2) - 1) >> chl2;
	const unsigned grid = (unsigned)((n_chunks + 255) / 256);
	hipStream_t s = (hipStream_t)stream;
	const unsigned mg = deemph_magic(a);
	const char *pick = rxgpu_knob("RXGPU_SCAN_T");                       /* "1": always scan_t, "0": scan_r wherever it applies (tests) */
	/* (256-sample chunks -- a = 19 at 240 kHz, BASELINE configs[0] -- always take scan_t: the register form reads every chunk once where scan_t
	 * reads the tails twice, 0.43 instead of 0.74 GB per 4 GiB of capture at ds = 5, but at 145 VGPRs per wave it took 1.2 ms instead of 0.66 and
	 * the pipelined step did not move: round 4, A/B in one process; the instantiation went in round 6) */
	if (chl2 == 7 && (pick ? pick[0] == '0' : M >= (1ull << 25))) {
		/* 128-sample chunks of a LONG run (the small-decimation chains, where the audio stages' traffic counts): the chunk in
		 * registers, the warm-up from the neighbouring lane; 63 chunks per wave.  Short runs keep scan_t: behind the big-ds
		 * decimator (56 VGPRs x 8 waves per SIMD) a wave of this kernel (81 VGPRs) waits for TWO of its waves to leave, and the
		 * audio chain of the headline run doubles (A/B at ds=118: 3 % on the pipelined step) */
		const unsigned rgrid = (unsigned)(((n_chunks + 62) / 63 + 3) / 4);
		if (group == 16)
			hipLaunchKernelGGL((k_fm_deemph_scan_r<16>), dim3(rgrid), dim3(256), 0, s, pcm_t, M, a, mg, warm, lo0, gap_w, (uint4 *)ctab, dev);
		else
			hipLaunchKernelGGL((k_fm_deemph_scan_r<64>), dim3(rgrid), dim3(256), 0, s, pcm_t, M, a, mg, warm, lo0, gap_w, (uint4 *)ctab, dev);
		LAUNCH_RET();
	}
#define GO(GS, CL) hipLaunchKernelGGL((k_fm_deemph_scan_t<GS, CL>), dim3(grid), dim3(256), 0, s, pcm_t, M, a, mg, warm, lo0, gap_w, (uint4 *)ctab, dev)
	if (group == 16) { if (chl2 == 7) GO(16, 7); else GO(16, 8); }
	else { if (chl2 == 7) GO(64, 7); else GO(64, 8); }
#undef GO
	LAUNCH_RET();
}

extern "C" int rxk_fm_deemph_up0(void *stream, u64 n_chunks, int group, const void *ctab, int *p_tab, int *p_lo, int *p_gap)
{
	const u64 parents = (n_chunks + DEEMPH_FAN - 1) / DEEMPH_FAN;
	const u64 threads = parents * group;
	hipLaunchKernelGGL(k_fm_deemph_up0, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
	                   n_chunks, group, (const uint4 *)ctab, p_tab, p_lo, p_gap);
	LAUNCH_RET();
}

extern "C" int rxk_fm_deemph_down0(void *stream, u64 n_chunks, const void *ctab, const int *p_start, int *start)
{
	const u64 parents = (n_chunks + DEEMPH_FAN - 1) / DEEMPH_FAN;
	hipLaunchKernelGGL(k_fm_deemph_down0, dim3((unsigned)((parents + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
	                   n_chunks, (const uint4 *)ctab, p_start, start);
	LAUNCH_RET();
}

extern "C" int rxk_fm_deemph_apply_rs_t(void *stream, const int16_t *pcm_t, u64 M, int a, int chl2, const int *start, int fast, int slow,
                                        int16_t *out, rxk_fm_dev *dev)
{
	if (!M)
		return 0;
	const u64 n_chunks = (M + (1u << chl2) - 1) >> chl2;
	const int ratio = fast / slow;
	// the reciprocal rounded UP: (int)((float)sum * rinv) is C's truncating sum / ratio for |sum| <= 34 * 32768, ratio <= 32
	const float rinv = __builtin_nextafterf((float)(1.0 / (double)ratio), __builtin_inff());
	// outputs one wave can produce: 64 chunks' worth of input, +1 window finished for a neighbour, +1 rounding
	const int wcap = ((int)((((u64)64 << chl2) * (u64)slow) / (u64)fast) + 6) & ~1;       /* + the spare element in front, even */
	// small workgroups: about 12 KiB of staging each (2 waves at the wbfm ratios), so that one finds room beside the
	// decimator's workgroups of the next run, which fill most of a CU's LDS
	int wpb = 4;
	while (wpb > 1 && (size_t)wpb * wcap * sizeof(int) > 12800)
		wpb >>= 1;
	const size_t lds = (size_t)wpb * wcap * sizeof(int);
	if (lds > 65536)
		return -1;
	const unsigned grid = (unsigned)((n_chunks + 64 * wpb - 1) / (64 * wpb));
	hipStream_t s = (hipStream_t)stream;
	const unsigned mg = deemph_magic(a);
	if (chl2 == 7)
		hipLaunchKernelGGL((k_fm_deemph_apply_rs_t<7>), dim3(grid), dim3(64 * wpb), lds, s, pcm_t, M, a, mg, start, fast, slow, rinv, wcap, out, dev);
	else
		hipLaunchKernelGGL((k_fm_deemph_apply_rs_t<8>), dim3(grid), dim3(64 * wpb), lds, s, pcm_t, M, a, mg, start, fast, slow, rinv, wcap, out, dev);
	LAUNCH_RET();
}

extern "C" int rxk_fm_deemph_serial(void *stream, const int16_t *pcm, u64 M, int a, int16_t *y, rxk_fm_dev *dev)
{
	hipLaunchKernelGGL(k_fm_deemph_serial, dim3(1), dim3(64), 0, (hipStream_t)stream, pcm, M, a, y, dev);
	LAUNCH_RET();
}

extern "C" int rxk_fm_resample(void *stream, const int16_t *y, u64 n, int fast, int slow, u64 J, int16_t *out, rxk_fm_dev *dev)
{
	hipLaunchKernelGGL(k_fm_resample, dim3((unsigned)((J + 1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, n, fast, slow, J, out, dev);
	LAUNCH_RET();
}

// A few bytes from one place to another as ONE WAVE.  hipMemcpyAsync of 4..240 bytes becomes a blit kernel whose workgroup
// waits for room while an HBM-bound kernel fills the chip -- rocprofv3 showed the 4-byte copy of the flag count sitting for a
// millisecond in front of the audio stages, and the next run's decimator waiting for those.  dst may be pinned host memory.
// a device buffer into its page-locked host mirror (16-byte aligned both sides): 16-byte units, the odd bytes at the end one by one
__global__ __launch_bounds__(256) void k_copy_mirror(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, unsigned n)
{
	const unsigned units = n >> 4;
	for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u)
		reinterpret_cast<uint4 *>(dst)[u] = reinterpret_cast<const uint4 *>(src)[u];
	if (blockIdx.x == 0 && threadIdx.x < (n & 15u))
		dst[(units << 4) + threadIdx.x] = src[(units << 4) + threadIdx.x];
}

__global__ void k_copy_small(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, unsigned n)
{
	for (unsigned i = threadIdx.x; i < n; i += 64)
		dst[i] = src[i];
}

extern "C" int rxk_copy_mirror(void *stream, void *dst, const void *src, unsigned bytes)
{
	if (!bytes)
		return 0;
	const unsigned grid = (bytes / 16 + 255) / 256;
	hipLaunchKernelGGL(k_copy_mirror, dim3(grid ? (grid > 64 ? 64 : grid) : 1), dim3(256), 0, (hipStream_t)stream, (uint8_t *)dst, (const uint8_t *)src, bytes);
	LAUNCH_RET();
}

extern "C" int rxk_copy_small(void *stream, void *dst, const void *src, unsigned bytes)
{
	if (!bytes)
		return 0;
	hipLaunchKernelGGL(k_copy_small, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint8_t *)dst, (const uint8_t *)src, bytes);
	LAUNCH_RET();
}

extern "C" int rxk_fm_carry_advance(void *stream, rxk_fm_dev *dev, int advance, int *snap)
{
	hipLaunchKernelGGL(k_fm_carry_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, dev, advance, snap);
	LAUNCH_RET();
}

extern "C" int rxk_fm_audio_carry(void *stream, rxk_fm_dev *dev, const int *snap)
{
	hipLaunchKernelGGL(k_fm_audio_carry, dim3(1), dim3(1), 0, (hipStream_t)stream, dev, snap);
	LAUNCH_RET();
}

extern "C" int rxk_fm_passthrough_carry(void *stream, rxk_fm_dev *dev, int deemph_off, int resample_off)
{
	hipLaunchKernelGGL(k_fm_passthrough_carry, dim3(1), dim3(1), 0, (hipStream_t)stream, dev, deemph_off, resample_off);
	LAUNCH_RET();
}

extern "C" int rxk_fm_fifth_pass(void *stream, const void *in, int in_is_raw, int prescaled, int rotate, u64 n_blocks,
                                 unsigned n_in, unsigned in_stride, uint32_t *out, unsigned out_stride,
                                 const int16_t *hist_in, int16_t *hist_out)
{
	const unsigned n_out = (n_in + 1) / 2;
	if (!n_blocks || !n_out)
		return 0;
	const dim3 grid((n_out + 255) / 256, (unsigned)(n_blocks < 65535 ? n_blocks : 65535));
	hipStream_t s = (hipStream_t)stream;
	if (!in_is_raw)
		hipLaunchKernelGGL((k_fm_fifth_pass<false, true, false>), grid, dim3(256), 0, s, in, n_blocks, n_in, in_stride, out, out_stride, hist_in, hist_out);
	else if (prescaled)
		hipLaunchKernelGGL((k_fm_fifth_pass<true, true, false>), grid, dim3(256), 0, s, in, n_blocks, n_in, in_stride, out, out_stride, hist_in, hist_out);
	else if (rotate)
		hipLaunchKernelGGL((k_fm_fifth_pass<true, false, true>), grid, dim3(256), 0, s, in, n_blocks, n_in, in_stride, out, out_stride, hist_in, hist_out);
	else
		hipLaunchKernelGGL((k_fm_fifth_pass<true, false, false>), grid, dim3(256), 0, s, in, n_blocks, n_in, in_stride, out, out_stride, hist_in, hist_out);
	LAUNCH_RET();
}

extern "C" int rxk_fm_droop(void *stream, const uint32_t *in, u64 M, const int *fir, const int16_t *hist_in,
                            int16_t *hist_out, uint32_t *out)
{
	if (!M)
		return 0;
	hipLaunchKernelGGL(k_fm_droop, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, M, fir, hist_in, hist_out, out);
	LAUNCH_RET();
}

extern "C" int rxk_fm_rdc(void *stream, const int16_t *iq, u64 n_blocks, u64 n_per_block, int prescaled, int rotate,
                          int rdc_block_const, int *state, long long *sums, int *avg, int16_t *out)
{
	if (!n_blocks || !n_per_block)
		return 0;
	hipStream_t s = (hipStream_t)stream;
	const u64 T = n_blocks * n_per_block;
	hipError_t e = hipMemsetAsync(sums, 0, (size_t)n_blocks * 16, s);
	if (e != hipSuccess)
		return (int)e;
	hipLaunchKernelGGL(k_fm_rdc_sums, dim3((unsigned)(n_blocks * RDC_PARTS)), dim3(256), 0, s, (const uint32_t *)iq, n_per_block, prescaled, (i64 *)sums);
	/* scaled samples are at most 128 in magnitude: |v + a c| <= 128 (c + 1) */
	hipLaunchKernelGGL(k_fm_rdc_scan, dim3(2), dim3(64), 0, s, (const i64 *)sums, n_blocks, (int)n_per_block, rdc_block_const, dc_div_magic(rdc_block_const + 1, 32768ll * (rdc_block_const + 1)), state, avg);
	if (out)                                             /* (NULL: the decimator subtracts the averages itself, rxk_fm_decimate_rdc) */
		hipLaunchKernelGGL(k_fm_rdc_apply, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, (const uint32_t *)iq, T, n_per_block, prescaled, rotate,
		                   avg, (uint32_t *)out);
	LAUNCH_RET();
}

extern "C" int rxk_fm_post_downsample(void *stream, const int16_t *in, u64 n_out, int step, int16_t *out)
{
	if (!n_out)
		return 0;
	hipLaunchKernelGGL(k_fm_post_downsample, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, n_out, step, out);
	LAUNCH_RET();
}

// The same with input and second output in HOST memory the device can address (page-locked: rxgpu_pin / rxgpu_dropin_pin): the callback's block
// crosses PCIe inside this launch -- 16-byte reads of the raw block, 16-byte writes of the scaled one to HBM (for full_demod) and back to the
// caller's buffer -- instead of in two DMA transfers around a kernel (three stream operations, each with its own latency: 47 us for 1 MiB).
__global__ __launch_bounds__(256) void k_fm_prestage_zc(const uint32_t *__restrict__ in, unsigned n, int rotate, uint32_t *__restrict__ out_dev,
                                                        uint32_t *__restrict__ out_host)
{
	// two samples per thread, 8-byte pieces: buf16[] sits 8 bytes off a 16-byte boundary in struct dongle_state (rtl_fm.c:128-147)
	const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
	const unsigned i0 = 2 * v;
	if (i0 >= n)
		return;
	if (i0 + 2 <= n) {
		const uint2 w = *reinterpret_cast<const uint2 *>(in + i0);
		const uint32_t ww[2] = {w.x, w.y};
		uint32_t r[2];
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const int i = scale_cs16(lo16(ww[k])), q = scale_cs16(hi16(ww[k]));
			int ri = i, rq = q;
			if (rotate) {
				switch ((i0 + k) & 3u) {
				case 1: ri = -q; rq = i; break;
				case 2: ri = -i; rq = -q; break;
				case 3: ri = q; rq = -i; break;
				default: break;
				}
			}
			r[k] = pack_iq(ri, rq);
		}
		const uint2 o = make_uint2(r[0], r[1]);
		*reinterpret_cast<uint2 *>(out_dev + i0) = o;
		*reinterpret_cast<uint2 *>(out_host + i0) = o;
		return;
	}
	int ri, rq;
	load_rot<false>(in, i0, rotate ? i0 : 0u, ri, rq);
	const uint32_t o = pack_iq(ri, rq);
	out_dev[i0] = o;
	out_host[i0] = o;
}

extern "C" int rxk_fm_prestage_zc(void *stream, const int16_t *in_host, unsigned n_complex, int rotate, int16_t *out_dev, int16_t *out_host)
{
	if (!n_complex)
		return 0;
	const unsigned vecs = (n_complex + 1) / 2;
	hipLaunchKernelGGL(k_fm_prestage_zc, dim3((vecs + 255) / 256), dim3(256), 0, (hipStream_t)stream,
	                   (const uint32_t *)in_host, n_complex, rotate, (uint32_t *)out_dev, (uint32_t *)out_host);
	LAUNCH_RET();
}

extern "C" int rxk_fm_prestage(void *stream, const int16_t *in, unsigned n_complex, int rotate, int16_t *out)
{
	if (!n_complex)
		return 0;
	hipLaunchKernelGGL(k_fm_prestage, dim3((n_complex + 255) / 256), dim3(256), 0, (hipStream_t)stream,
	                   (const uint32_t *)in, n_complex, rotate, (uint32_t *)out);
	LAUNCH_RET();
}

// the seam histories of a fused group alone (k_fm_fifth_seams), for callers that run it ahead of the group on another stream;
// rxk_fm_fifth_fused with hist_in == NULL then skips it
extern "C" int rxk_fm_fifth_seams(void *stream, const void *in, int stage2, int rotate, u64 n_blocks, unsigned n, int fuse,
                                  const int16_t *hist_in, int16_t *hist_out, uint32_t *seams)
{
	const u64 seam_threads = (n_blocks + 1) * 16;
	const unsigned sgrid = (unsigned)((seam_threads + 255) / 256);
	const uint32_t *p = (const uint32_t *)in;
	hipStream_t s = (hipStream_t)stream;
	if (fuse >= 4 && !stage2) {                                  /* the four- / five-pass register kernels' layout: 5 * fuse dwords per block */
		const unsigned sgrid4 = (unsigned)(((n_blocks + 1) * 32 + 255) / 256);
		if (fuse == 4) {
			if (rotate) hipLaunchKernelGGL((k_fm_fifth_seams<true, false, 4>), dim3(sgrid4), dim3(256), 0, s, p, n_blocks, n, fuse, hist_in, seams, hist_out);
			else hipLaunchKernelGGL((k_fm_fifth_seams<false, false, 4>), dim3(sgrid4), dim3(256), 0, s, p, n_blocks, n, fuse, hist_in, seams, hist_out);
		} else {
			if (rotate) hipLaunchKernelGGL((k_fm_fifth_seams<true, false, 5>), dim3(sgrid4), dim3(256), 0, s, p, n_blocks, n, fuse, hist_in, seams, hist_out);
			else hipLaunchKernelGGL((k_fm_fifth_seams<false, false, 5>), dim3(sgrid4), dim3(256), 0, s, p, n_blocks, n, fuse, hist_in, seams, hist_out);
		}
		LAUNCH_RET();
	}
	if (stage2) hipLaunchKernelGGL((k_fm_fifth_seams<false, true>), dim3(sgrid), dim3(256), 0, s, p, n_blocks, n, fuse, hist_in, seams, hist_out);
	else if (rotate) hipLaunchKernelGGL((k_fm_fifth_seams<true, false>), dim3(sgrid), dim3(256), 0, s, p, n_blocks, n, fuse, hist_in, seams, hist_out);
	else hipLaunchKernelGGL((k_fm_fifth_seams<false, false>), dim3(sgrid), dim3(256), 0, s, p, n_blocks, n, fuse, hist_in, seams, hist_out);
	LAUNCH_RET();
}

// `fuse` (1..3) fifth_order passes in one LDS-tiled launch.  stage2 == 0: raw cs16 in (scale + rotate, packed int16
// arithmetic); stage2 != 0: packed level samples in (int arithmetic), hist_* already offset to the first pass done
extern "C" int rxk_fm_fifth_fused(void *stream, const void *in, int stage2, int rotate, u64 n_blocks, unsigned n, int fuse,
                                  const int16_t *hist_in, int16_t *hist_out, uint32_t *seams, uint32_t *out)
{
	hipStream_t s = (hipStream_t)stream;
	const unsigned tiles = n / FF_RAW;
	const unsigned tpw = tiles % 16 == 0 ? 16 : tiles % 8 == 0 ? 8 : tiles % 4 == 0 ? 4 : tiles % 2 == 0 ? 2 : 1;   // tiles one workgroup walks
	const u64 seam_threads = (n_blocks + 1) * 16;
	const unsigned sgrid = (unsigned)((seam_threads + 255) / 256);
	const unsigned grid = (unsigned)(n_blocks * (tiles / tpw));
	const uint32_t *p = (const uint32_t *)in;
#define SEAMS(RT, S2) hipLaunchKernelGGL((k_fm_fifth_seams<RT, S2>), dim3(sgrid), dim3(256), 0, s, p, n_blocks, n, fuse, hist_in, seams, hist_out)
	/* the raw stage's workgroups take a fifth of the CU's LDS each (15 KiB of tiles + this pad): with eight per CU the kernel is no
	 * faster, and the later passes / discriminator / audio stages of the previous run on the other stream wait for wave slots
	 * (A/B in one process, -F ds=128 pipelined: 0.92 -> 0.98 TSample/s) */
	const size_t pad = stage2 ? 0 : 17000;
#define FUSED(F, RT, S2) hipLaunchKernelGGL((k_fm_fifth_fused<F, RT, S2, false>), dim3(grid), dim3(256), pad, s, p, n, tiles, tpw, seams, out, n, n >> F)
#define GO(RT, S2) do { if (hist_in) SEAMS(RT, S2); if (fuse == 1) FUSED(1, RT, S2); else if (fuse == 2) FUSED(2, RT, S2); else FUSED(3, RT, S2); } while (0)
	/* four passes on the raw capture: the register kernel, 16 samples per lane (five -- 1/32 out -- bought nothing more: round 3).  A group of three
	 * passes that is not the whole chain (k_fm_fifth_regn<., 3, DD>, rxk_fm_fifth_dd) stays with the LDS-tiled kernel below: 3-5 % ahead there (A/B) */
	if (!stage2 && fuse == 4) {
		const unsigned tiles_r = ((n >> fuse) + FR_OUT - 1) / FR_OUT;
		/* one tile per wave: walking two or four with the next one's loads in flight (what the whole-chain kernel below does) made this
		 * one, which has half the arithmetic per byte, 5-10 % slower (A/B, -F ds=128: 1730 / 1823 / 1908 us per step) */
		const unsigned wgs_per_block = (tiles_r + 3) / 4;
		const u64 total = n_blocks * (u64)wgs_per_block;
		if (total > 0xfffffff0ull)
			return (int)hipErrorInvalidValue;
		const unsigned rgrid = (unsigned)((total + 7) / 8 * 8);
		const unsigned sgridn = (unsigned)(((n_blocks + 1) * 32 + 255) / 256);
#define SEAMN(RT, LVV) hipLaunchKernelGGL((k_fm_fifth_seams<RT, false, LVV>), dim3(sgridn), dim3(256), 0, s, p, n_blocks, n, fuse, hist_in, seams, hist_out)
#define REGK(RT, LVV, T) hipLaunchKernelGGL((k_fm_fifth_regn<RT, LVV, 0, T>), dim3(rgrid), dim3(256), 0, s, p, n, tiles_r, wgs_per_block, (unsigned)total, seams, out, \
		                                    (const uint32_t *)nullptr, 0, 0, 0, 0, 0, (int16_t *)nullptr, 0, (uint32_t *)nullptr)
#define REGN(RT, LVV) REGK(RT, LVV, 1)
#define GON(LVV) do { if (rotate) { if (hist_in) SEAMN(true, LVV); REGN(true, LVV); } else { if (hist_in) SEAMN(false, LVV); REGN(false, LVV); } } while (0)
		GON(4);
#undef GON
#undef REGN
#undef REGK
#undef SEAMN
		LAUNCH_RET();
	}
	if (stage2) GO(false, true);
	else if (rotate) GO(true, false);
	else GO(false, false);
#undef GO
#undef FUSED
#undef SEAMS
	LAUNCH_RET();
}

// the whole -F chain of a three-pass cascade in one launch (k_fm_fifth_regn<.., 3, DD>): seams from rxk_fm_fifth_seams (fuse = 3), tails from
// rxk_fm_fifth_tails; fir == NULL: no droop FIR.  n % RXK_FIFTH_TILE == 0
extern "C" int rxk_fm_fifth_dd(void *stream, const void *in, int rotate, u64 n_blocks, unsigned n, int fuse, const uint32_t *seams, const uint32_t *tails,
                               const int *fir, int16_t *pcm, int pcm_chl2, uint32_t *edges)
{
	if (fuse != 3)
		return (int)hipErrorInvalidValue;
	hipStream_t s = (hipStream_t)stream;
	const uint32_t *p = (const uint32_t *)in;
	const unsigned tiles_r = ((n >> fuse) / 4 + FR_OUT - 1) / FR_OUT;
	/* two tiles per wave, the second one's loads in flight behind the first one's arithmetic (A/B round 3: 1 / 2 / 4 tiles, two is ahead); short
	 * blocks: one */
	const unsigned twn = tiles_r >= 8 ? 2u : 1u;
	const unsigned wgs_per_block = (tiles_r + 4 * twn - 1) / (4 * twn);
	const u64 total = n_blocks * (u64)wgs_per_block;
	if (total > 0xfffffff0ull)
		return (int)hipErrorInvalidValue;
	const unsigned rgrid = (unsigned)((total + 7) / 8 * 8);
#define DDK(RT, D, T) hipLaunchKernelGGL((k_fm_fifth_regn<RT, 3, D, T>), dim3(rgrid), dim3(256), 0, s, p, n, tiles_r, wgs_per_block, (unsigned)total, seams, (uint32_t *)nullptr, \
		                                 tails, fir ? fir[1] : 0, fir ? fir[2] : 0, fir ? fir[3] : 0, fir ? fir[4] : 0, fir ? fir[5] : 0, pcm, pcm_chl2, edges)
#define DDT(RT, D) do { if (twn == 2) DDK(RT, D, 2); else DDK(RT, D, 1); } while (0)
	if (fir) { if (rotate) DDT(true, 2); else DDT(false, 2); }
	else { if (rotate) DDT(true, 1); else DDT(false, 1); }
#undef DDT
#undef DDK
	LAUNCH_RET();
}

extern "C" int rxk_fm_fifth_tails(void *stream, const void *in, int rotate, u64 n_blocks, unsigned n, int fuse, const int16_t *droop_in, int16_t *droop_out,
                                  uint32_t *tails)
{
	if (fuse != 3)
		return (int)hipErrorInvalidValue;
	const unsigned grid = (unsigned)(((n_blocks + 1) * 16 + 255) / 256);
	if (rotate) hipLaunchKernelGGL((k_fm_fifth_tails<true, 3>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)in, n_blocks, n, droop_in, droop_out, tails);
	else hipLaunchKernelGGL((k_fm_fifth_tails<false, 3>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)in, n_blocks, n, droop_in, droop_out, tails);
	LAUNCH_RET();
}

extern "C" int rxk_fm_dd_edges(void *stream, const uint32_t *edges, u64 n_blocks, u64 K, int16_t *pcm, int pcm_chl2, rxk_fm_dev *dev, rxk_flag_rec *flag_list,
                               int *flag_cnt, int flag_all)
{
	hipLaunchKernelGGL(k_fm_dd_edges, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, edges, n_blocks, K, pcm, pcm_chl2, dev, flag_list,
	                   flag_cnt, flag_all);
	LAUNCH_RET();
}

extern "C" int rxk_fm_fifth_lit(void *stream, const int16_t *in, int16_t *out, int L, const int16_t *hist_in, int16_t *hist_out)
{
	const int K = L > 4 ? 1 + (L - 1) / 4 : 1;                     // the I half has at least as many outputs as the Q half
	hipLaunchKernelGGL(k_fm_fifth_lit, dim3((unsigned)((K + 255) / 256), 2), dim3(256), 0, (hipStream_t)stream, in, out, L, hist_in, hist_out);
	LAUNCH_RET();
}

extern "C" int rxk_fm_droop_lit(void *stream, const int16_t *in, int16_t *out, int L, const int *fir, const int16_t *hist_in, int16_t *hist_out)
{
	const int n = (L > 2 ? L : 2) / 2 + 2;                          // the filtered samples of the longer half and the few entries behind them
	hipLaunchKernelGGL(k_fm_droop_lit, dim3((unsigned)((n + 255) / 256), 2), dim3(256), 0, (hipStream_t)stream, in, out, L, fir, hist_in, hist_out);
	LAUNCH_RET();
}

extern "C" int rxk_fm_squelch_lit(void *stream, int16_t *lp, int L, int level, int *below, int *sr_out)
{
	hipLaunchKernelGGL(k_fm_squelch_lit, dim3(1), dim3(256), 0, (hipStream_t)stream, lp, L, level, below, sr_out);
	LAUNCH_RET();
}

extern "C" int rxk_fm_demod_lit(void *stream, const int16_t *lp, int L, int mode, int custom_atan, int output_scale, int16_t *pcm,
                                unsigned long long m0, rxk_fm_dev *dev, int pre_from_out, rxk_flag_rec *flag_list, int *flag_cnt,
                                const int *atan_lut, int flag_all)
{
	const int n = mode == RXK_LIT_RAW ? L : L / 2;
	if (n > 0) {
		hipLaunchKernelGGL(k_fm_demod_lit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, lp, L, mode, custom_atan, output_scale,
		                   pcm, (u64)m0, dev, pre_from_out, flag_list, flag_cnt, atan_lut, flag_all);
		if (hipGetLastError() != hipSuccess)
			return (int)hipErrorLaunchFailure;
	}
	if (mode == RXK_LIT_FM && L >= 2)
		hipLaunchKernelGGL(k_fm_pre_lit, dim3(1), dim3(1), 0, (hipStream_t)stream, lp, L, dev);
	LAUNCH_RET();
}

extern "C" int rxk_fm_squelch(void *stream, uint32_t *lp, rxk_fm_blocks blk, int level, int *below, int *sr_out)
{
	hipLaunchKernelGGL(k_fm_squelch, dim3((unsigned)blk.n_blocks), dim3(256), 0, (hipStream_t)stream, lp, blk, level, below, sr_out);
	LAUNCH_RET();
}

extern "C" int rxk_fm_simple_demod(void *stream, const uint32_t *lp, u64 M, int mode, int output_scale, int16_t *pcm)
{
	if (!M)
		return 0;
	hipLaunchKernelGGL(k_fm_simple_demod, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, lp, M, mode, output_scale, pcm);
	LAUNCH_RET();
}

extern "C" int rxk_fm_dc_block(void *stream, int16_t *y, u64 M, rxk_fm_blocks blk, int adc_block_const, long long *sums,
                               int *avgs, rxk_fm_dev *dev)
{
	hipStream_t s = (hipStream_t)stream;
	hipLaunchKernelGGL(k_fm_dc_sums, dim3((unsigned)blk.n_blocks), dim3(256), 0, s, y, blk, (i64 *)sums);
	/* demodulated samples are int16: |v + dc c| <= 32768 (c + 1) */
	hipLaunchKernelGGL(k_fm_dc_scan, dim3(1), dim3(64), 0, s, (const i64 *)sums, blk, adc_block_const, dc_div_magic(adc_block_const + 1, 32768ll * (adc_block_const + 1)), avgs, dev);
	hipLaunchKernelGGL(k_fm_dc_apply, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, y, M, blk, avgs);
	LAUNCH_RET();
}

extern "C" int rxk_ch_fused_ok(int bin_e, u64 wpb, int custom_atan, int n_channels)
{
	const int wpg = ch_wpg(bin_e);
	/* the run of windows a workgroup walks: what k_ch_demod(sparse) then skips over */
	return (bin_e >= 8 && bin_e <= 12 && custom_atan == 1 && wpb % wpg == 0) ? wpg * ch_gpw(wpg, wpb) : 0;
}

extern "C" int rxk_ch_fft(void *stream, const int16_t *iq, u64 total_windows, int bin_e, const uint32_t *twiddle,
                          int first_bin, int n_channels, uint32_t *chan_lp, int fused, int16_t *out, u64 out_stride, int *pre_out)
{
	if (!total_windows)
		return 0;
	if (bin_e >= 8 && bin_e <= 12) {
		const int CH_WPG = ch_wpg(bin_e);
		const int GPW = fused ? fused / CH_WPG : ch_gpw(CH_WPG, 0);
		/* N <= 1024: one transpose area (k_ch_fftR); rows of RXK_FFT_XROW dwords (fft_exchange's layout), the permuted twiddle copy, the staging */
		const size_t shm = (size_t)((bin_e <= 10 ? 1 : 2) * 256 * RXK_FFT_XROW + 8 * ((1 << (bin_e - 4)) + 8) + n_channels * (CH_WPG + 3)) * 4;
		const u64 run = (u64)CH_WPG * GPW;
		const unsigned grid = (unsigned)(((total_windows + run - 1) / run + 7) / 8 * 8);   /* XCD-contiguous order inside the kernel */
		hipStream_t s = (hipStream_t)stream;
		const uint32_t *p = (const uint32_t *)iq;
#define GOF__(MM, FU, TW, WP) do { if (shm > 64 * 1024) (void)hipFuncSetAttribute((const void *)k_ch_fftR<MM, FU, TW, WP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm); \
		hipLaunchKernelGGL((k_ch_fftR<MM, FU, TW, WP>), dim3(grid), dim3(256), shm, s, p, total_windows, twiddle + (1 << (MM - 1)), first_bin, n_channels, chan_lp, \
		                   out, out_stride, pre_out, GPW); } while (0)
#define GOF(MM, FU) GOF__(MM, FU, true, 16)
#define GOC(MM) do { if (fused) GOF(MM, true); else GOF(MM, false); } while (0)
		switch (bin_e) {
		case 8: GOC(8); break; case 9: GOC(9); break; case 10: GOC(10); break; case 11: GOC(11); break; default: GOC(12); break;
		}
#undef GOC
#undef GOF
#undef GOF__
		LAUNCH_RET();
	}
	int wpg = bin_e >= 13 ? 1 : (8192 >> bin_e);
	const size_t shm = ((size_t)wpg << bin_e) * 4;
	static size_t allowed = 64 * 1024;
	if (shm > allowed) {
		(void)hipFuncSetAttribute((const void *)k_ch_fft, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
		allowed = 144 * 1024;
	}
	const unsigned grid = (unsigned)((total_windows + wpg - 1) / wpg);
	hipLaunchKernelGGL(k_ch_fft, dim3(grid), dim3(256), shm, (hipStream_t)stream, (const uint32_t *)iq, total_windows, bin_e, wpg,
	                   twiddle, first_bin, n_channels, chan_lp);
	LAUNCH_RET();
}

extern "C" int rxk_ch_nco(void *stream, const int16_t *iq, u64 total_windows, int bin_e, const uint32_t *tw_full, int first_bin, int n_channels,
                          uint32_t *chan_lp)
{
	if (!total_windows)
		return 0;
	const int wpg = 4;
	const size_t shm = (size_t)2 * ((size_t)1 << bin_e) * 4;
	if (shm > 64 * 1024)
		(void)hipFuncSetAttribute((const void *)k_ch_nco<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
	hipLaunchKernelGGL(k_ch_nco<0>, dim3((unsigned)((total_windows + wpg - 1) / wpg), (unsigned)((n_channels + 255) / 256)), dim3(256), shm, (hipStream_t)stream,
	                   (const uint32_t *)iq, total_windows, bin_e, tw_full, first_bin, n_channels, chan_lp, wpg);
	LAUNCH_RET();
}

extern "C" int rxk_ch_demod(void *stream, const uint32_t *chan_lp, u64 total_windows, u64 wpb, int n_channels, int custom_atan,
                            const int *pre_in, int *pre_out, int16_t *out, u64 out_stride, rxk_fm_dev *dev, u64 *flag_list, int sparse)
{
	const u64 total = sparse ? (u64)n_channels * ((total_windows + sparse - 1) / sparse) : (u64)n_channels * total_windows;
	if (!total)
		return 0;
	hipLaunchKernelGGL(k_ch_demod, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, chan_lp, total_windows, wpb,
	                   n_channels, custom_atan, pre_in, pre_out, out, out_stride, dev, flag_list, sparse,
	                   rxgpu_knob("RXGPU_FLAG_ALL") ? atoi(rxgpu_knob("RXGPU_FLAG_ALL")) : 0);
	LAUNCH_RET();
}

extern "C" int rxk_ch_squelch(void *stream, uint32_t *chan_lp, u64 total_windows, u64 wpb, int n_channels, int level, uint8_t *below, int *sr_out)
{
	const u64 n_blocks = total_windows / wpb, segs = (u64)n_channels * n_blocks;
	if (!segs)
		return 0;
	if (wpb >= CH_SQ_WAVE_MIN) {
		hipLaunchKernelGGL(k_ch_squelch_wave, dim3((unsigned)((segs + 3) / 4)), dim3(256), 0, (hipStream_t)stream, chan_lp, total_windows, wpb, n_blocks,
		                   n_channels, level, below, sr_out);
		LAUNCH_RET();
	}
	const dim3 grid((unsigned)((segs + 255) / 256));
	if (wpb % 4 == 0 && total_windows % 4 == 0)
		hipLaunchKernelGGL(k_ch_squelch<true>, grid, dim3(256), 0, (hipStream_t)stream, chan_lp, total_windows, wpb, n_blocks, n_channels, level, below, sr_out);
	else
		hipLaunchKernelGGL(k_ch_squelch<false>, grid, dim3(256), 0, (hipStream_t)stream, chan_lp, total_windows, wpb, n_blocks, n_channels, level, below, sr_out);
	LAUNCH_RET();
}

extern "C" int rxk_ch_simple_demod(void *stream, const uint32_t *chan_lp, u64 total_windows, int n_channels, int mode, int output_scale,
                                   const int *pre_in, int *pre_out, int16_t *out, u64 out_stride)
{
	if (!total_windows || !n_channels)
		return 0;
	hipLaunchKernelGGL(k_ch_simple_demod, dim3((unsigned)((total_windows + 255) / 256), (unsigned)n_channels), dim3(256), 0, (hipStream_t)stream, chan_lp,
	                   total_windows, mode, output_scale, pre_in, pre_out, out, out_stride);
	LAUNCH_RET();
}

extern "C" int rxk_ch_gate(void *stream, const uint8_t *below, u64 n_blocks, int n_channels, int conseq, int zero, const int *hits_in, int *hits_out,
                           uint8_t *gate)
{
	hipLaunchKernelGGL(k_ch_gate, dim3((unsigned)((n_channels + 63) / 64)), dim3(64), 0, (hipStream_t)stream, below, n_blocks, n_channels, conseq, zero,
	                   hits_in, hits_out, gate);
	LAUNCH_RET();
}

extern "C" int rxk_ch_gate_zero(void *stream, int16_t *out, u64 out_stride, u64 J, u64 wpb, u64 n_blocks, int n_channels, int fast, int slow, u64 p0,
                                const uint8_t *gate)
{
	if (!J)
		return 0;
	hipLaunchKernelGGL(k_ch_gate_zero, dim3((unsigned)((J + 255) / 256), (unsigned)n_channels), dim3(256), 0, (hipStream_t)stream, out, out_stride, J,
	                   wpb, n_blocks, fast, slow, p0, gate);
	LAUNCH_RET();
}

// deemph_filter (rtl_fm.c:667-682) + low_pass_real (389-409) on ONE short row (the drop-in's single blocks: a thousand samples behind ds = 118),
// k_ch_audio's scheme with the row in LDS and the chunk length cut loose from the warm-up: k_ch_audio walks global memory sample by sample
// (46 us for 1 110 samples: every step of every chain waits for its load) and gives each thread a chunk of at least `warm` samples (ten threads
// busy).  Here thread 0 takes the first `warm` samples from the carried state, every other thread a chunk of C samples behind them, warmed up
// on the `warm` samples before its own (two trajectories from the ends of the int16 range, as there), then the chunk tables are walked by one
// thread and every chunk is replayed from its exact start.  a > 64, a == 1 or a carried state outside int16 (serial): one thread, the
// reference's own expression.  W <= row_cap samples (the launcher's LDS size).  row: in (demodulated) / out (result); audio: {avg, now_lpr,
// prev_lpr_index} in, the same three out at audio + 3.
template <bool EVEN, bool D24>
__global__ __launch_bounds__(256) void k_fm_row_audio(const int16_t *row_g, int16_t *row_out, unsigned W, int deemph, int a, unsigned magic, int bias,
                                                      int warm, int serial, int fast, int slow, unsigned J, const int *audio, int *audio_out,
                                                      int16_t *__restrict__ row_h, int *__restrict__ audio_h, const uint32_t *__restrict__ hdr,
                                                      uint32_t *__restrict__ hdr_h, unsigned hdr_words)
{
	extern __shared__ __attribute__((aligned(16))) int16_t ra_row[];       // [W] the samples, then (in place) the de-emphasised ones
	__shared__ uint4 tab[256];
	__shared__ int start[256];
	const int tid = threadIdx.x;
	for (unsigned i = tid; i < W; i += 256)
		ra_row[i] = row_g[i];
	// row_h, audio_h, hdr_h: the page-locked host mirror of the result row, the three audio carries and k_fm_block_dd's header -- what the
	// caller reads after the stream's synchronisation, no copy operation in between
	for (unsigned i = tid; i < hdr_words; i += 256)
		hdr_h[i] = hdr[i];
	const int avg_in = audio[0];
	__syncthreads();
	if (deemph) {
		const int h = a / 2, xoff = h + bias * a;
		// chunk 0 = [0, w0), chunk t >= 1 = [w0 + (t - 1) C, w0 + t C): at most 255 of them
		const unsigned w0 = serial ? W : min((unsigned)warm, W);
		// (the walk over the chunk tables is one thread's, ~250 cycles per table, a step of a chain ~50: chunks of 48 balance the two at W ~ 1000)
		unsigned Cn = (W - w0 + 254) / 255;
		Cn = Cn < 48 ? 48 : ((Cn + 7) & ~7u);                 // a multiple of 8: the chunk starts stay 8-byte aligned for the uint2 reads below
		const int active = 1 + (int)((W - w0 + Cn - 1) / Cn);
		const unsigned b = tid ? w0 + (unsigned)(tid - 1) * Cn : 0u, e = tid ? min(W, b + Cn) : w0;
		if (tid < active && !serial) {
			int lo, hi;
			if (tid == 0) {
				lo = hi = avg_in;
			} else {
				lo = -32768; hi = 32767;
				// four samples per LDS read (b and warm are multiples of 8): a chain step is five instructions, a read's latency a hundred cycles
				for (unsigned i = b - (unsigned)warm; i < b; i += 4) {
					const uint2 v = *reinterpret_cast<const uint2 *>(&ra_row[i]);
					const int xs[4] = {lo16(v.x), hi16(v.x), lo16(v.y), hi16(v.y)};
#pragma unroll
					for (int q = 0; q < 4; q++) {
						lo = deemph_step_d<EVEN, D24>(lo, xs[q] + xoff, xs[q], magic, bias);
						hi = deemph_step_d<EVEN, D24>(hi, xs[q] + xoff, xs[q], magic, bias);
					}
				}
			}
			int gap = hi - lo;
			if (gap > 63) gap = 63;                               // excluded by `warm`
			const int lo_start = lo;
			int cnt = gap + 1;
			u64 mask = (((u64)1 << gap) - 1);
			unsigned i = b;
			for (; i + 4 <= e; i += 4) {
				const uint2 v = *reinterpret_cast<const uint2 *>(&ra_row[i]);
				const int xs[4] = {lo16(v.x), hi16(v.x), lo16(v.y), hi16(v.y)};
#pragma unroll
				for (int q = 0; q < 4; q++)
					deemph_track<EVEN, D24>(lo, cnt, mask, xs[q], a, xoff, magic, bias);
			}
			for (; i < e; i++)
				deemph_track<EVEN, D24>(lo, cnt, mask, (int)ra_row[i], a, xoff, magic, bias);
			tab[tid] = make_uint4((uint32_t)lo_start, ((uint32_t)lo & 0xffffu) | ((uint32_t)gap << 16), (uint32_t)mask, (uint32_t)(mask >> 32));
		}
		__syncthreads();
		if (tid == 0) {
			int s = avg_in;
			if (!serial) {
#pragma unroll 4
				for (int t = 0; t < active; t++) {
					start[t] = s;
					s = ctab_apply(tab[t], s);
				}
				audio_out[0] = s; audio_h[0] = s;
			} else {
				for (unsigned i = 0; i < W; i++) {                // any a, any state: the reference's own expression
					const int d = (int)ra_row[i] - s;
					s += d > 0 ? (d + h) / a : (d - h) / a;
					ra_row[i] = (int16_t)s;
				}
				audio_out[0] = s; audio_h[0] = s;
			}
		}
		__syncthreads();
		if (tid < active && !serial) {
			int s = start[tid];
			unsigned i = b;
			for (; i + 4 <= e; i += 4) {
				const uint2 v = *reinterpret_cast<const uint2 *>(&ra_row[i]);
				const int xs[4] = {lo16(v.x), hi16(v.x), lo16(v.y), hi16(v.y)};
				int ys[4];
#pragma unroll
				for (int q = 0; q < 4; q++) {
					s = deemph_step_d<EVEN, D24>(s, xs[q] + xoff, xs[q], magic, bias);
					ys[q] = s;
				}
				*reinterpret_cast<uint2 *>(&ra_row[i]) = make_uint2(pack_iq(ys[0], ys[1]), pack_iq(ys[2], ys[3]));
			}
			for (; i < e; i++) {
				const int x = ra_row[i];
				s = deemph_step_d<EVEN, D24>(s, x + xoff, x, magic, bias);
				ra_row[i] = (int16_t)s;
			}
		}
		__syncthreads();
	} else if (tid == 0) {
		audio_out[0] = avg_in; audio_h[0] = avg_in;
	}
	if (slow > 0) {
		const u64 p0 = (u64)audio[2];
		const int ratio = fast / slow;
		for (unsigned j = tid; j < J; j += 256) {
			const u64 wb = j ? lpr_end(j - 1, fast, slow, p0) : 0, we = lpr_end(j, fast, slow, p0);
			int sum = j ? 0 : audio[1];
			for (u64 i = wb; i < we; i++)
				sum += ra_row[i];
			if (row_out)
				row_out[j] = (int16_t)(sum / ratio);
			row_h[j] = (int16_t)(sum / ratio);
		}
		if (tid == 0) {
			const u64 wb = J ? lpr_end(J - 1, fast, slow, p0) : 0;
			int sum = J ? 0 : audio[1];
			for (u64 i = wb; i < W; i++)
				sum += ra_row[i];
			const int pl = (int)(p0 + (u64)W * (u64)slow - (u64)J * (u64)fast);
			audio_out[1] = sum; audio_h[1] = sum;
			audio_out[2] = pl; audio_h[2] = pl;
		}
	} else {
		for (unsigned i = tid; i < W; i += 256) {
			if (row_out && (deemph || row_out != row_g))
				row_out[i] = ra_row[i];
			row_h[i] = ra_row[i];
		}
		if (tid == 0) { const int nl = audio[1], pl = audio[2]; audio_out[1] = nl; audio_out[2] = pl; audio_h[1] = nl; audio_h[2] = pl; }
	}
}

extern "C" int rxk_fm_row_audio(void *stream, const int16_t *row, int16_t *row_out, unsigned W, int deemph, int a, int warm, int serial, int fast, int slow,
                                unsigned J, const int *audio, int *audio_out, int16_t *row_h, int *audio_h, const void *hdr, void *hdr_h, unsigned hdr_words)
{
	if (!W)
		return 0;
	hipStream_t s = (hipStream_t)stream;
	const unsigned mg = deemph ? deemph_magic_u(a) : 0u;
	const int bias = deemph ? bias_for(a) : 0;
	const size_t lds = ((size_t)W * 2 + 15) & ~(size_t)15;
#define GO(EV, D) hipLaunchKernelGGL((k_fm_row_audio<EV, D>), dim3(1), dim3(256), lds, s, row, row_out, W, deemph, a, mg, bias, warm, serial, fast, slow, J, audio, audio_out, \
		row_h, audio_h, (const uint32_t *)hdr, (uint32_t *)hdr_h, hdr_words)
	if (deemph && deemph_d24u(a)) { if (a & 1) GO(false, true); else GO(true, true); }
	else { if (!deemph || (a & 1)) GO(false, false); else GO(true, false); }
#undef GO
	LAUNCH_RET();
}

extern "C" int rxk_fm_block_dd(void *stream, const int16_t *blk, unsigned n, int ds, int p0, int now_r, int now_j, int pre_r, int pre_j,
                               int custom_atan, uint32_t *lp, uint32_t *lp_host, int16_t *pcm, int16_t *keep, rxk_blk_out *out, int *audio_in, int avg,
                               int now_lpr, int prev_lpr_index)
{
	const unsigned long long M = ((unsigned long long)p0 + n) / (unsigned long long)ds;
	unsigned grid = (unsigned)((M + 1 + 3) / 4);
	if (grid > 2048)
		grid = 2048;
	hipLaunchKernelGGL(k_fm_block_dd, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)blk, n, ds, p0, now_r, now_j, pre_r, pre_j,
	                   custom_atan, rxgpu_knob("RXGPU_FLAG_ALL") ? atoi(rxgpu_knob("RXGPU_FLAG_ALL")) : 0, lp, lp_host, pcm, keep, out, audio_in, avg, now_lpr, prev_lpr_index);
	LAUNCH_RET();
}

// chunk length and count of the segmented form for a row of W samples; 0 chunks = the row is too short (or too long for CHA_MAX_SEG segments of
// 256 chunks at a sane chunk length): k_ch_audio serves it
extern "C" unsigned rxk_ch_audio_chunks(u64 W, int warm, unsigned *chunk_out)
{
	u64 chunk = (u64)((warm + 7) & ~7);
	const u64 need = (W + 256u * CHA_MAX_SEG - 1) / (256u * CHA_MAX_SEG);
	if (chunk < need)
		chunk = (need + 7) & ~(u64)7;
	if (chunk < 8)
		chunk = 8;
	if (chunk >= 48)
		chunk = (chunk + 63) & ~(u64)63;                              // whole 128-byte lines per lane and turn (k_cha_track)
	const u64 n = (W + chunk - 1) / chunk;
	if (chunk_out)
		*chunk_out = (unsigned)chunk;
	return (n < 64 || chunk > 4096) ? 0u : (unsigned)n;
}

// LDS int16 slots a workgroup of k_cha_replay_rs stages its outputs in (256 chunks' worth + the window finished for a neighbour + rounding);
// 0: the fused form does not fit (the caller keeps k_ch_audio)
static unsigned cha_rs_cap(unsigned chunk, int fast, int slow)
{
	const u64 cap = (256ull * chunk * (u64)slow) / (u64)fast + 4;
	return cap * 2 <= 40960 ? (unsigned)cap : 0u;
}

// can the (segment, channel) form serve rows of W samples (deemph on, a in 2..64, carried states inside int16)?  It reads the demodulated rows
// from one buffer and writes the audio to another.
extern "C" int rxk_ch_audio_seg_ok(u64 W, int warm, int fast, int slow)
{
	unsigned chunk = 0;
	if (!rxk_ch_audio_chunks(W, warm, &chunk) || W >= 0x7fffffffull)
		return 0;
	return slow > 0 ? (cha_rs_cap(chunk, fast, slow) != 0 && fast / slow >= 1 && fast / slow <= 32) : 1;      /* windows shorter than any chunk */
}

// ctab: n_channels * n_chunks tables; seg_start: n_channels * n_chunks ints (every chunk's start state).  in_rows != out_rows.
extern "C" int rxk_ch_audio_seg(void *stream, const int16_t *in_rows, u64 in_stride, int16_t *out_rows, u64 out_stride, u64 W, int n_channels, int a,
                                int warm, int fast, int slow, const int *audio_in, int *audio_out, void *ctab_v, int *seg_start)
{
	uint4 *ctab = (uint4 *)ctab_v;
	unsigned chunk = 0;
	const unsigned n_chunks = rxk_ch_audio_chunks(W, warm, &chunk);
	if (!n_chunks || !rxk_ch_audio_seg_ok(W, warm, fast, slow) || (const int16_t *)out_rows == in_rows)
		return (int)hipErrorInvalidValue;
	hipStream_t s = (hipStream_t)stream;
	const unsigned mg = deemph_magic_u(a);
	const int bias = bias_for(a);
	const unsigned n_seg = (n_chunks + 255) / 256;
	const dim3 grid(n_seg, (unsigned)n_channels);
	const int ratio = slow > 0 ? fast / slow : 1;
	// the reciprocal rounded UP: (int)((float)sum * rinv) is C's truncating sum / ratio for |sum| <= 34 * 32768, ratio <= 32 (rxk_fm_deemph_apply_rs_t)
	const float rinv = (slow > 0 && ratio <= 32) ? __builtin_nextafterf((float)(1.0 / (double)ratio), __builtin_inff()) : 0.0f;
	const unsigned cap = slow > 0 ? cha_rs_cap(chunk, fast, slow) : 0u;
#define GO(EV, D) do { \
		hipLaunchKernelGGL((k_cha_track<EV, D>), grid, dim3(256), 0, s, in_rows, in_stride, W, a, mg, bias, warm, chunk, n_chunks, audio_in, ctab); \
		hipLaunchKernelGGL(k_cha_walk, dim3((unsigned)n_channels), dim3(64 * n_seg), (size_t)n_chunks * 20, s, ctab, n_chunks, audio_in, audio_out, seg_start); \
		if (slow > 0) \
			hipLaunchKernelGGL((k_cha_replay_rs<EV, D>), grid, dim3(256), (size_t)cap * 2, s, in_rows, in_stride, W, a, mg, bias, chunk, n_chunks, seg_start, \
			                   fast, slow, ratio, rinv, audio_in, audio_out, out_rows, out_stride, cap); \
		else \
			hipLaunchKernelGGL((k_cha_replay<EV, D>), grid, dim3(256), 0, s, in_rows, in_stride, W, a, mg, bias, chunk, n_chunks, seg_start, \
			                   audio_in, audio_out, out_rows, out_stride); } while (0)
	if (deemph_d24u(a)) { if (a & 1) GO(false, true); else GO(true, true); }
	else { if (a & 1) GO(false, false); else GO(true, false); }
#undef GO
	LAUNCH_RET();
}

extern "C" int rxk_ch_audio(void *stream, int16_t *rows, u64 row_stride, u64 W, int n_channels, int deemph, int a, int warm, int serial,
                            int fast, int slow, u64 J, const int *audio_in, int *audio_out, int16_t *y_rows, u64 y_stride)
{
	if (!W || !n_channels)
		return 0;
	hipStream_t s = (hipStream_t)stream;
	const unsigned mg = deemph ? deemph_magic_u(a) : 0u;
	const int bias = deemph ? bias_for(a) : 0;
#define GO(EV, D) hipLaunchKernelGGL((k_ch_audio<EV, D>), dim3((unsigned)n_channels), dim3(256), 0, s, rows, row_stride, W, deemph, a, mg, bias, warm, serial, \
		fast, slow, J, audio_in, audio_out, y_rows, y_stride)
	if (deemph && deemph_d24u(a)) { if (a & 1) GO(false, true); else GO(true, true); }
	else { if (!deemph || (a & 1)) GO(false, false); else GO(true, false); }
#undef GO
	LAUNCH_RET();
}

extern "C" int rxk_fm_droop_disc(void *stream, const uint32_t *in, u64 M, const int *fir, const int16_t *hist_in, int16_t *hist_out,
                                 uint32_t *lp_out, u64 uniform_k, int16_t *pcm, int pcm_chl2, rxk_fm_dev *dev, rxk_flag_rec *flag_list,
                                 int *flag_cnt, int flag_all)
{
	if (!M)
		return 0;
	const unsigned grid = (unsigned)(((M + 3) / 4 + 255) / 256);
	hipStream_t s = (hipStream_t)stream;
	if (!fir)                                              /* no filter: the discriminator alone, four outputs per thread (lp_out unused: the input IS lowpassed[]) */
		hipLaunchKernelGGL((k_fm_droop_disc<false, false>), dim3(grid), dim3(256), 0, s, in, M, fir, hist_in, hist_out, (uint32_t *)nullptr, uniform_k, pcm, pcm_chl2, dev,
		                   flag_list, flag_cnt, flag_all);
	else if (lp_out)
		hipLaunchKernelGGL((k_fm_droop_disc<true>), dim3(grid), dim3(256), 0, s, in, M, fir, hist_in, hist_out, lp_out, uniform_k, pcm, pcm_chl2, dev,
		                   flag_list, flag_cnt, flag_all);
	else
		hipLaunchKernelGGL((k_fm_droop_disc<false>), dim3(grid), dim3(256), 0, s, in, M, fir, hist_in, hist_out, lp_out, uniform_k, pcm, pcm_chl2, dev,
		                   flag_list, flag_cnt, flag_all);
	LAUNCH_RET();
}

// rx_power's downsample_iq (rtl_power.c:656-662): `fuse` (1..3) stateless fifth_order passes over n_bufs independent buffers of n
// complex samples (n % RXK_FIFTH_TILE == 0) in one LDS-tiled launch; strides in complex samples
extern "C" int rxk_pw_fifth_fused(void *stream, const int16_t *in, unsigned long long n_bufs, unsigned n, unsigned in_stride, int fuse,
                                  int16_t *out, unsigned out_stride)
{
	hipStream_t s = (hipStream_t)stream;
	const unsigned tiles = n / FF_RAW;
	const unsigned tpw = tiles % 16 == 0 ? 16 : tiles % 8 == 0 ? 8 : tiles % 4 == 0 ? 4 : tiles % 2 == 0 ? 2 : 1;
	const unsigned grid = (unsigned)(n_bufs * (tiles / tpw));
	const uint32_t *p = (const uint32_t *)in;
	uint32_t *o = (uint32_t *)out;
#define FUSED(F) hipLaunchKernelGGL((k_fm_fifth_fused<F, false, true, true>), dim3(grid), dim3(256), 0, s, p, n, tiles, tpw, nullptr, o, in_stride, out_stride)
	if (fuse == 1) FUSED(1); else if (fuse == 2) FUSED(2); else FUSED(3);
#undef FUSED
	LAUNCH_RET();
}

// four stateless passes (+ the droop FIR: fir = cic_9_tables[4] on the device, or NULL) in registers, the buffers' dc sums accumulated into sums[2 * buffer],
// [2 * buffer + 1] (zeroed by the caller; NULL: none).  n % 64 == 0, n >= 256; strides in complex samples, multiples of 4; out 16-byte aligned
// lv = 2, 3 or 4 passes.  wave_part (sums != NULL): rxk_pw_fifth_regn_parts(n_bufs, n, lv) int pairs of scratch, one per wave
extern "C" unsigned long long rxk_pw_fifth_regn_parts(unsigned long long n_bufs, unsigned n, int lv)
{
	const unsigned tiles_r = ((n >> lv) / 4 + FR_OUT - 1) / FR_OUT;
	const unsigned twn = tiles_r >= 4 * 2 ? 2 : 1;
	return n_bufs * (unsigned long long)((tiles_r + 4 * twn - 1) / (4 * twn)) * 4ull;
}

template <int LV>
static int pw_fifth_regn_launch(hipStream_t s, const int16_t *in, unsigned long long n_bufs, unsigned n, unsigned in_stride, const int *fir_dev, const int *fir_host,
                                int16_t *out, unsigned out_stride, long long *sums, int *wave_part)
{
	constexpr int TW = 2;
	const unsigned tiles_r = ((n >> LV) / 4 + FR_OUT - 1) / FR_OUT;
	const unsigned twn = tiles_r >= 4 * TW ? TW : 1;
	const unsigned wgs_per_block = (tiles_r + 4 * twn - 1) / (4 * twn);
	const u64 total = n_bufs * (u64)wgs_per_block;
	if (total > 0xfffffff0ull || n_bufs > 0x7fffffffull)
		return (int)hipErrorInvalidValue;
	const unsigned rgrid = (unsigned)((total + 7) / 8 * 8);
	const uint32_t *p = (const uint32_t *)in;
	uint32_t *o = (uint32_t *)out;
	const unsigned fgrid = (unsigned)((n_bufs + 3) / 4);
	const int f1 = fir_host ? fir_host[1] : 0, f2 = fir_host ? fir_host[2] : 0, f3 = fir_host ? fir_host[3] : 0, f4 = fir_host ? fir_host[4] : 0, f5 = fir_host ? fir_host[5] : 0;
#define PWR(FI, T) hipLaunchKernelGGL((k_pw_fifth_regn<LV, FI, T>), dim3(rgrid), dim3(256), 0, s, p, n, in_stride, tiles_r, wgs_per_block, (unsigned)total, o, out_stride, \
		                              f1, f2, f3, f4, f5, sums ? (int2 *)wave_part : (int2 *)nullptr)
	if (fir_host) {
		if (twn == TW) PWR(true, TW); else PWR(true, 1);
		hipLaunchKernelGGL((k_pw_fifth_fix<LV, true>), dim3(fgrid), dim3(256), 0, s, p, (unsigned)n_bufs, in_stride, o, out_stride, fir_dev, (i64 *)sums, (const int2 *)wave_part, wgs_per_block * 4u);
	} else {
		if (twn == TW) PWR(false, TW); else PWR(false, 1);
		hipLaunchKernelGGL((k_pw_fifth_fix<LV, false>), dim3(fgrid), dim3(256), 0, s, p, (unsigned)n_bufs, in_stride, o, out_stride, fir_dev, (i64 *)sums, (const int2 *)wave_part, wgs_per_block * 4u);
	}
#undef PWR
	LAUNCH_RET();
}

extern "C" int rxk_pw_fifth_regn(void *stream, const int16_t *in, unsigned long long n_bufs, unsigned n, unsigned in_stride, int lv, const int *fir_dev, const int *fir_host,
                                 int16_t *out, unsigned out_stride, long long *sums, int *wave_part)
{
	if ((sums && !wave_part) || lv < 2 || lv > 4)
		return (int)hipErrorInvalidValue;
	hipStream_t s = (hipStream_t)stream;
	if (lv == 2) return pw_fifth_regn_launch<2>(s, in, n_bufs, n, in_stride, fir_dev, fir_host, out, out_stride, sums, wave_part);
	if (lv == 3) return pw_fifth_regn_launch<3>(s, in, n_bufs, n, in_stride, fir_dev, fir_host, out, out_stride, sums, wave_part);
	return pw_fifth_regn_launch<4>(s, in, n_bufs, n, in_stride, fir_dev, fir_host, out, out_stride, sums, wave_part);
}
