// fm_part_chan.inc -- part of fm_kernels.hip (one translation unit; included there, in this order: helpers, decimate, audio, cascade, chan, launch).
// the channeliser (extension): FFT bank, NCO mode, per-channel demodulation and audio stages
// ------------------------------------------------------------------ channeliser (extension)

// BASELINE configs[4] / SURVEY section 8(f) rank 2 -- not in the reference; specified from its primitives
// (include/rxgpu.h, "rx_fm: channeliser"): every window of N capture samples through fix_fft
// (rtl_power.c:264-320), bin first_bin+c of successive windows = channel c's lowpassed[] stream.
// One workgroup transforms `wpg` consecutive windows side by side in LDS (the stage index maths
// of the radix-2 network does not care that the array holds several aligned windows) and writes
// the selected bins as [channel][window], wpg windows contiguous per channel.
__global__ __launch_bounds__(256) void k_ch_fft(const uint32_t *__restrict__ iq, u64 total_windows, int bin_e, int wpg,
                                                const uint32_t *__restrict__ twiddle, int first_bin, int n_channels,
                                                uint32_t *__restrict__ chan_lp)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t x[];
	const int n = 1 << bin_e, tot = wpg << bin_e;
	const u64 w0 = (u64)blockIdx.x * wpg;
	for (int e = threadIdx.x; e < tot; e += 256) {
		const int win = e >> bin_e, j = e & (n - 1);
		const uint32_t v = (w0 + win < total_windows) ? iq[((w0 + win) << bin_e) + j] : 0u;
		x[(win << bin_e) + (int)(__brev((unsigned)j) >> (32 - bin_e))] = v;      // rtl_power.c:275-290
	}
	__syncthreads();
	for (int s = 0; s < bin_e; s++) {                                             // rtl_power.c:291-318
		const int half = 1 << s;
		for (int b = threadIdx.x; b < tot / 2; b += 256) {
			const int t = b & (half - 1);
			const int lo_i = ((b >> s) << (s + 1)) | t;
			uint32_t lo = x[lo_i], hi = x[lo_i + half];
			butterfly(lo, hi, twiddle[t << (bin_e - 1 - s)]);
			x[lo_i] = lo;
			x[lo_i + half] = hi;
		}
		__syncthreads();
	}
	for (int idx = threadIdx.x; idx < n_channels * wpg; idx += 256) {
		const int c = idx / wpg, win = idx - c * wpg;
		if (w0 + win < total_windows)
			chan_lp[(u64)c * total_windows + w0 + win] = x[(win << bin_e) + ((first_bin + c) & (n - 1))];
	}
}

// The same with the register-blocked transform (fft_device.h), N = 2^M, M = 8..12: N/16 threads per
// window, 256/(N/16) windows side by side, CH_WPG windows per workgroup so that every channel's
// outputs leave as one contiguous segment.
// windows per workgroup: 32 while the [n_channels][wpg] staging fits beside the transform buffers, else 16
static inline int ch_wpg(int bin_e)
{
	(void)bin_e;
	return 16;                                               /* round 3, 256 channels: 387-392 GS/s with 16 windows per group, 367-375 with 32; 8 no better */
}
// groups of WPG windows a workgroup walks (round 4): the twiddle copy, the slot arithmetic and the addresses are set up once per run of
// WPG * GPW windows, and the last window of a group stays in LDS as the next group's predecessor -- only a RUN's first window is left to
// k_ch_demod(sparse).  The largest of 4, 2, 1 that divides the callback block's windows.
static inline int ch_gpw(int wpg, u64 wpb)
{
	int g = 4;
	while (g > 1 && wpb % (u64)(wpg * g))
		g >>= 1;
	return g;
}
// FUSED: also fm_demod (-A fast) for every window but the run's first, straight from the LDS copy of the bins; then
// only the entries k_ch_demod(sparse) reads are stored in chan_lp (each run's first and last window).  Needs the
// callback blocks to be whole runs of WPG * GPW windows, so that a block's first (libm) window is a run's first.
// Staging rows: [channel][1 + WPG] -- column 0 holds the previous group's last window -- padded to WPG + 3 dwords (odd: the 64 channels a
// wave's store touches fall on 32 banks twice, not on two banks).  The tail's thread (c, k) keeps its window k for every channel it visits:
// its pointers advance by a constant, nothing is divided.
template <int M, bool FUSED, bool TWL = true, int WPG = 16>
__global__ __launch_bounds__(256) void k_ch_fftR(const uint32_t *__restrict__ iq, u64 total_windows,
                                                 const uint32_t *__restrict__ twiddle, int first_bin, int n_channels,
                                                 uint32_t *__restrict__ chan_lp, int16_t *__restrict__ out, u64 out_stride,
                                                 int *__restrict__ pre_out, int GPW)
{
	typedef fft_geom<M> G;
	constexpr int N = G::N, TPF = G::TPF, FPW = 256 / TPF, S = WPG + 3, CPI = 256 / WPG;
	// N <= 1024: a window's N/16 threads are lanes of one wave, its transposes need no workgroup barrier (fft_sync) and -- a wave's LDS
	// instructions being in order -- no second transpose area either: 20 KB less LDS per workgroup, and the four waves run their windows
	// without waiting for each other (round 2: 72 KB and three barriers per window group left two barrier-coupled waves per SIMD)
	constexpr bool WAVE = TPF <= 64;
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	uint32_t *xa = lds, *xb = WAVE ? lds : lds + 256 * G::XROW;
	uint32_t *tl = lds + (WAVE ? 1 : 2) * 256 * G::XROW;     // the permuted twiddle copy (fft_device.h), G::TW_WORDS dwords
	uint32_t *outt = tl + G::TW_WORDS;                      // [n_channels][S]
	const int tid = threadIdx.x, fid = tid / TPF;
	const unsigned tq = tid % TPF;
	const int RUN = WPG * GPW;
	// XCD-contiguous order: workgroup b runs on XCD b % 8, every XCD takes one contiguous eighth of the capture -- the 32-byte pieces that
	// neighbouring runs write into a channel's row then meet in ONE L2
	const unsigned per = gridDim.x >> 3, run_i = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
	const u64 w0 = (u64)run_i * RUN;
	if (w0 >= total_windows)
		return;
	const u64 w_last = total_windows - 1;
	fft_tw_fill<M>(tl, twiddle, tid, 256);
	unsigned ta[3][4];
	fft_tw_addr_all<M>(tq, ta);
	// the next windows are requested while these are transformed (round 4); past the capture's end the last window again (never stored)
	uint32_t nxt[16];
	{
		const u64 w = w0 + fid < w_last ? w0 + fid : w_last;
		const uint32_t *src = iq + (w << M) + tq;
#pragma unroll
		for (int r = 0; r < 16; r++)
			nxt[r] = src[r * TPF];
	}
	const int k = tid & (WPG - 1), c0 = tid / WPG;
	__syncthreads();                                        // the twiddle copy
#pragma unroll 1
	for (int it = 0; it < RUN; it += FPW) {
		uint32_t v[16];
#pragma unroll
		for (int r = 0; r < 16; r++)
			v[r] = nxt[r];
		if (it + FPW < RUN) {
			const u64 wn = w0 + it + FPW + fid, w = wn < w_last ? wn : w_last;
			const uint32_t *src = iq + (w << M) + tq;
#pragma unroll
			for (int r = 0; r < 16; r++)
				nxt[r] = src[r * TPF];
		}
		fft_reg<M, !WAVE, TWL>(v, tq, xa + fid * TPF * G::XROW, xb + fid * TPF * G::XROW, twiddle, tl, ta);
		const int col = (it & (WPG - 1)) + fid + 1;
#pragma unroll
		for (int r = 0; r < 16; r++) {
			const unsigned bin = __brev((tq << 4) | (unsigned)r) >> (32 - M);
			const unsigned c = (bin - (unsigned)first_bin) & (N - 1);
			if (c < (unsigned)n_channels)
				outt[c * S + col] = v[r];
		}
		const bool run_done = w0 + it + FPW >= total_windows;    // workgroup-uniform: a ragged last run (never in FUSED form)
		if (((it + FPW) & (WPG - 1)) && !run_done)
			continue;
		// a group is complete
		__syncthreads();
		const int g = it / WPG;                                 // (it + FPW) / WPG - 1
		const u64 w = w0 + (u64)g * WPG + k;
		if (w < total_windows) {
			const bool run_first = g == 0 && k == 0;
			const bool run_last = k == WPG - 1 && g == GPW - 1;
			const bool keep = !FUSED || run_first || run_last;
			const bool last = w == w_last;
			// FUSED: only what k_ch_demod(sparse) reads is kept, compact: [channel][run] first windows, then [channel][run] last windows
			const u64 n_runs = total_windows / (u64)RUN, lp_stride = FUSED ? n_runs : total_windows;
			uint32_t *lp = chan_lp + (u64)c0 * lp_stride + (FUSED ? (run_last ? (u64)n_channels * n_runs : 0) + run_i : w);
			int16_t *o = out + (u64)c0 * out_stride + w;
			const uint32_t *row = outt + c0 * S + k;
			for (int c = c0; c < n_channels; c += CPI, lp += (u64)CPI * lp_stride, o += (u64)CPI * out_stride, row += CPI * S) {
				const uint32_t a = row[1];
				if (keep)
					*lp = a;
				if (!FUSED)
					continue;
				const uint32_t b = row[0];
				if (last) {                                         // fm_demod's carry, rtl_fm.c:612-613
					pre_out[2 * c] = lo16(a);
					pre_out[2 * c + 1] = hi16(a);
				}
				if (!run_first) {
					int cr, cj;
					mul_conj_pk(a, b, cr, cj);
					*o = (int16_t)fast_atan2_dev<false>(cj, cr);
				}
				if (k == WPG - 1)
					outt[c * S] = a;                                // the next group's window -1 (read above by lane k == 0 of this wave, in order)
			}
		}
		if (run_done)
			break;
		__syncthreads();
	}
}

// The channeliser's second definition (SURVEY 8(f)2 to the letter; rxgpu_chan_params.nco): per channel an integer NCO, then low_pass
// (rtl_fm.c:351-371) at downsample = N.  The capture goes through the callback's scale (rtl_fm.c:845-848, no rotation); sample n of a
// window is multiplied by e^(-j 2 pi k n / N), k = (first_bin + c) mod N, with cos / sin from the reference's Sinewave table (nco_tw: the
// full period as packed (cos, sin), built on the host) and each of the four products rounded by FIX_MPY (rtl_power.c:256-262); low_pass
// sums the N mixed samples of a window in int and stores the sum as int16.  |scaled sample| <= 128, so a FIX_MPY result is at most 128 in
// magnitude and a mixed component 256: nothing wraps before low_pass's own int16 store.  One thread per channel, the window and the
// table in LDS (the sample is a broadcast read, the table index k * n mod N differs per lane): N^2-ish work -- 256 channels of 1024 cost
// ~50 times the fix_fft bank's butterflies -- which is why the bank is the default; this mode exists because the survey named it.
template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_ch_nco(const uint32_t *__restrict__ iq, u64 total_windows, int bin_e, const uint32_t *__restrict__ tw_full,
                                                int first_bin, int n_channels, uint32_t *__restrict__ chan_lp, int wpg)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t nco_sm[];      // [N] scaled window, [N] table
	const int n = 1 << bin_e;
	uint32_t *xs = nco_sm, *tw = nco_sm + n;
	for (int i = threadIdx.x; i < n; i += 256)
		tw[i] = tw_full[i];
	const unsigned c = blockIdx.y * 256u + threadIdx.x;
	const unsigned k = ((unsigned)first_bin + c) & (unsigned)(n - 1);
	for (int wi = 0; wi < wpg; wi++) {
		const u64 w = (u64)blockIdx.x * wpg + wi;
		if (w >= total_windows)
			break;
		__syncthreads();
		for (int i = threadIdx.x; i < n; i += 256) {
			const uint32_t v = iq[(w << bin_e) + i];
			xs[i] = pack_iq(scale_cs16(lo16(v)), scale_cs16(hi16(v)));
		}
		__syncthreads();
		int sr = 0, sj = 0;
		unsigned p = 0;
		for (int i = 0; i < n; i++) {
			const uint32_t x = xs[i], t = tw[p];
			p = (p + k) & (unsigned)(n - 1);
			const int xr = lo16(x), xi = hi16(x), co = lo16(t), si = hi16(t);
			const int rc = (xr * co + 16384) >> 15, is = (xi * si + 16384) >> 15;       // FIX_MPY: ((a*b >> 14) + 1) >> 1
			const int ic = (xi * co + 16384) >> 15, rs = (xr * si + 16384) >> 15;
			sr += rc + is;
			sj += ic - rs;
		}
		if (c < (unsigned)n_channels)
			chan_lp[(u64)c * total_windows + w] = pack_iq(sr, sj);                  // low_pass's int16 stores
	}
}

// fm_demod (rtl_fm.c:584-615) per channel: thread (c, t); the first window of every callback block
// goes through the libm discriminator like every block's first sample does in rx_fm
// sparse = run length of k_ch_fftR<FUSED> (0: dense): only the first window of every run, thread (c, run)
__global__ void k_ch_demod(const uint32_t *__restrict__ chan_lp, u64 total_windows, u64 wpb, int n_channels, int custom_atan,
                           const int *__restrict__ pre_in, int *__restrict__ pre_out, int16_t *__restrict__ out, u64 out_stride,
                           rxk_fm_dev *__restrict__ dev, u64 *__restrict__ flag_list, int sparse, int flag_all)
{
	u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
	u64 c, t;
	uint32_t a;
	int br, bj;
	if (sparse) {
		// the fused FFT kernel left [channel][run] first windows, then [channel][run] last windows
		const u64 runs = total_windows / (u64)sparse;
		if (gid >= (u64)n_channels * runs)
			return;
		c = gid / runs;
		const u64 r = gid - c * runs;
		t = r * (u64)sparse;
		a = chan_lp[gid];
		if (r) {
			const uint32_t b = chan_lp[(u64)n_channels * runs + gid - 1];
			br = lo16(b); bj = hi16(b);
		} else {
			br = pre_in[2 * c]; bj = pre_in[2 * c + 1];
		}
		gid = c * total_windows + t;                         // the flag list names samples, not slots
	} else {
		if (gid >= (u64)n_channels * total_windows)
			return;
		c = gid / total_windows; t = gid - c * total_windows;
		a = chan_lp[gid];
		if (t) {
			const uint32_t b = chan_lp[gid - 1];
			br = lo16(b); bj = hi16(b);
		} else {
			br = pre_in[2 * c]; bj = pre_in[2 * c + 1];
		}
	}
	const int ar = lo16(a), aj = hi16(a);
	const int cr = (int)((unsigned)ar * (unsigned)br + (unsigned)aj * (unsigned)bj);
	const int cj = (int)((unsigned)aj * (unsigned)br - (unsigned)ar * (unsigned)bj);
	int v;
	if (custom_atan == 0 || (t % wpb) == 0) {
		const double ang = atan2((double)cj, (double)cr);
		const double r = ang / 3.14159 * 16384.0;
		v = (int)r;
		if (r != 0.0 && (flag_forced(flag_all, gid) || fabs(r - rint(r)) < RXK_LIBM_WINDOW)) {
			const int idx = atomicAdd(&dev->flag_cnt, 1);
			if (idx < RXK_FLAG_CAP)
				flag_list[idx] = gid;
			if (flag_all >= 2)
				v ^= 0x55;                                       // $RXGPU_FLAG_ALL=2|3: only the host's re-evaluation can make it right
		}
	} else {
		v = fast_atan2_dev(cj, cr);
	}
	out[c * out_stride + t] = (int16_t)v;
	if (t == total_windows - 1) {
		pre_out[2 * c] = ar;
		pre_out[2 * c + 1] = aj;
	}
}

// ---- full_demod's power squelch and other demodulators per channel, the demod thread's gate (rxgpu_chan_params.mode .. squelch_zero).
// They work on the dense bins ([channel][window], every window stored): the fused -A fast kernel keeps too few of them.

// rtl_fm.c:781-790 with rms() 739-757 (step 1, over I and Q) on every (channel, callback block) segment of wpb bins: one thread per segment
// (a wave per segment of 64 bins spent its time in the reduction: 216 us per 1 GiB capture), k_fm_squelch's int64 sums and double expression.
// A quiet segment is zeroed in place: k_ch_demod's neighbour read at a block seam and the host's libm fix-ups (they re-read chan_lp) then see
// what fm_demod sees in the reference.  below / sr_out: [channel][block].  VEC: wpb and total_windows multiples of 4, 16-byte pieces
__device__ __forceinline__ void ch_sq_acc(uint32_t w, i64 &t, u64 &p)
{
	const int i = lo16(w), q = hi16(w);
	t += i + q;
	p += (u64)((unsigned)(i * i) + (unsigned)(q * q));          // <= 2^31: exact in 32 bits unsigned
}
// rms() (rtl_fm.c:739-757) from the block's sums in k_fm_squelch's double expression; true: below the level
__device__ __forceinline__ bool ch_sq_verdict(i64 t, i64 p, u64 wpb, int level, int &sr)
{
	const int len = (int)(2 * wpb);
	const double dc = (double)t / (double)len;              // (double)(t*step)/(double)len, step == 1
	const double lhs = (double)(t * 2) * dc;
	const double rhs = dc * dc * (double)len;
	const double v = ((double)p - (lhs - rhs)) / (double)len;
	sr = v >= 0.0 ? (int)isqrt_floor(v) : 0;
	return sr < level;
}
template <bool VEC>
__global__ __launch_bounds__(256) void k_ch_squelch(uint32_t *__restrict__ chan_lp, u64 total_windows, u64 wpb, u64 n_blocks, int n_channels, int level,
                                                    uint8_t *__restrict__ below, int *__restrict__ sr_out)
{
	const u64 seg = (u64)blockIdx.x * 256 + threadIdx.x;
	if (seg >= (u64)n_channels * n_blocks)
		return;
	const u64 c = seg / n_blocks, b = seg - c * n_blocks;
	uint32_t *lp = chan_lp + c * total_windows + b * wpb;
	i64 t = 0;
	u64 pu = 0;
	if (VEC) {
#pragma unroll 4
		for (u64 m = 0; m < wpb; m += 4) {
			const uint4 w = *reinterpret_cast<const uint4 *>(lp + m);
			ch_sq_acc(w.x, t, pu); ch_sq_acc(w.y, t, pu); ch_sq_acc(w.z, t, pu); ch_sq_acc(w.w, t, pu);
		}
	} else {
		for (u64 m = 0; m < wpb; m++)
			ch_sq_acc(lp[m], t, pu);
	}
	int sr;
	const bool quiet = ch_sq_verdict(t, (i64)pu, wpb, level, sr);
	below[seg] = quiet ? 1 : 0;
	sr_out[seg] = sr;
	if (quiet) {
		if (VEC)
			for (u64 m = 0; m < wpb; m += 4)
				*reinterpret_cast<uint4 *>(lp + m) = make_uint4(0u, 0u, 0u, 0u);
		else
			for (u64 m = 0; m < wpb; m++)
				lp[m] = 0;
	}
}

// The same for long blocks (wpb >= CH_SQ_WAVE_MIN windows: few channels, many windows per block -- a thread per segment would walk hundreds of KB
// alone): one wave per segment, lanes strided over it, the int64 sums reduced across the wave
#define CH_SQ_WAVE_MIN 512
__global__ __launch_bounds__(256) void k_ch_squelch_wave(uint32_t *__restrict__ chan_lp, u64 total_windows, u64 wpb, u64 n_blocks, int n_channels,
                                                         int level, uint8_t *__restrict__ below, int *__restrict__ sr_out)
{
	const u64 seg = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
	const unsigned lane = threadIdx.x & 63u;
	if (seg >= (u64)n_channels * n_blocks)                   // wave-uniform
		return;
	const u64 c = seg / n_blocks, b = seg - c * n_blocks;
	uint32_t *lp = chan_lp + c * total_windows + b * wpb;
	i64 t = 0;
	u64 pu = 0;
	for (u64 m = lane; m < wpb; m += 64)
		ch_sq_acc(lp[m], t, pu);
	i64 p = (i64)pu;
	for (int off = 32; off; off >>= 1) { t += __shfl_down(t, off); p += __shfl_down(p, off); }
	t = __shfl(t, 0);
	p = __shfl(p, 0);
	int sr;
	const bool quiet = ch_sq_verdict(t, p, wpb, level, sr);
	if (lane == 0) {
		below[seg] = quiet ? 1 : 0;
		sr_out[seg] = sr;
	}
	if (quiet)
		for (u64 m = lane; m < wpb; m += 64)
			lp[m] = 0;
}

// am_demod / usb_demod / lsb_demod / raw_demod (rtl_fm.c:617-665) on the dense bins, grid (windows, channel): no 64-bit division per sample;
// k_fm_simple_demod's arithmetic; raw: the bin as two int16 (rows of 2 * total_windows).  fm_demod's carry passes through: only fm_demod writes
// pre_r / pre_j
__global__ __launch_bounds__(256) void k_ch_simple_demod(const uint32_t *__restrict__ chan_lp, u64 total_windows, int mode, int output_scale,
                                                         const int *__restrict__ pre_in, int *__restrict__ pre_out, int16_t *__restrict__ out, u64 out_stride)
{
	const u64 t = (u64)blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
	if (t >= total_windows)
		return;
	const uint32_t w = chan_lp[c * total_windows + t];
	const int i = lo16(w), q = hi16(w);
	int16_t *o = out + c * out_stride;
	if (mode == RXK_LIT_RAW) {
		o[2 * t] = (int16_t)i;
		o[2 * t + 1] = (int16_t)q;
	} else {
		int v;
		if (mode == RXK_LIT_AM) {
			const int pw = (int)((unsigned)(i * i) + (unsigned)(q * q));    // may wrap at full scale, like the reference's int
			v = pw < 0 ? 0 : (int)(short)isqrt_floor((double)pw);           // (int16_t)sqrt(NaN) is 0 on x86
		} else {
			v = (int)(short)(mode == RXK_LIT_USB ? i + q : i - q);
		}
		o[t] = (int16_t)(v * output_scale);
	}
	if (t == 0) {
		pre_out[2 * c] = pre_in[2 * c];
		pre_out[2 * c + 1] = pre_in[2 * c + 1];
	}
}

// the demod thread's gate (rtl_fm.c:927-940) behind full_demod's count (781-790): one thread per channel walks the run's blocks in order --
// squelch_hits from the verdicts, gate 0 written / 1 dropped (the hair trigger clamps the count) / 2 zeroed -- and leaves its count for the
// next run on the device (hits_out: the next run's hits_in, like pre_out)
__global__ void k_ch_gate(const uint8_t *__restrict__ below, u64 n_blocks, int n_channels, int conseq, int zero, const int *__restrict__ hits_in,
                          int *__restrict__ hits_out, uint8_t *__restrict__ gate)
{
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= n_channels)
		return;
	const uint8_t *bl = below + (u64)c * n_blocks;
	uint8_t *g = gate + (u64)c * n_blocks;
	int hits = hits_in[c];
	// sixteen verdicts per load where the rows allow it, the next sixteen requested before these are walked (a byte per step waited for
	// every load: 101 us for 2048 blocks)
	const bool vec = (n_blocks & 15u) == 0 && (((size_t)bl | (size_t)g) & 15u) == 0;
	const u64 nv = vec ? n_blocks : 0;
	uint4 nxt = nv ? *reinterpret_cast<const uint4 *>(bl) : make_uint4(0u, 0u, 0u, 0u);
	for (u64 b0 = 0; b0 < nv; b0 += 16) {
		const uint4 cur = nxt;
		if (b0 + 16 < nv)
			nxt = *reinterpret_cast<const uint4 *>(bl + b0 + 16);
		const uint32_t in[4] = {cur.x, cur.y, cur.z, cur.w};
		uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
		for (int k = 0; k < 16; k++) {
			hits = ((in[k >> 2] >> (8 * (k & 3))) & 0xffu) ? (int)((unsigned)hits + 1u) : 0;
			uint32_t v = 0;
			if (hits > conseq) {
				if (zero)
					v = 2;
				else {
					hits = conseq + 1;                      // hair trigger
					v = 1;
				}
			}
			o[k >> 2] |= v << (8 * (k & 3));
		}
		*reinterpret_cast<uint4 *>(g + b0) = make_uint4(o[0], o[1], o[2], o[3]);
	}
	for (u64 b = nv; b < n_blocks; b++) {
		hits = bl[b] ? (int)((unsigned)hits + 1u) : 0;
		uint8_t v = 0;
		if (hits > conseq) {
			if (zero)
				v = 2;
			else {
				hits = conseq + 1;
				v = 1;
			}
		}
		g[b] = v;
	}
	hits_out[c] = hits;
}

// squelch_zero behind the audio stages: output j of a channel belongs to the block of the sample that emitted it -- with low_pass_real
// (slow > 0) input sample lpr_end(j) - 1 (the phase p0 in front of the run is the same in every channel), else sample j
__global__ void k_ch_gate_zero(int16_t *__restrict__ out, u64 out_stride, u64 J, u64 wpb, u64 n_blocks, int fast, int slow, u64 p0,
                               const uint8_t *__restrict__ gate)
{
	const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
	if (j >= J)
		return;
	const u64 i = slow > 0 ? lpr_end(j, (u64)fast, (u64)slow, p0) - 1 : j;
	const u64 b = i / wpb;
	if (b < n_blocks && gate[c * n_blocks + b] == 2)
		out[c * out_stride + j] = 0;
}


// Per-channel audio stages of the channeliser: deemph_filter (rtl_fm.c:667-682) and low_pass_real (389-409) on every
// channel's demodulated stream, each channel with its own carried state like a demod_state of its own (rtl_fm.c:189
// "multiple of these, eventually").  One workgroup per channel.  De-emphasis: every thread takes a contiguous chunk of the
// channel's samples, narrows the possible start states on the `warm` samples before it (two extreme trajectories), tracks
// lowest candidate + merge mask through its chunk (deemph_track, any a up to 64), thread 0 walks the chunk tables from the
// carried state, and every thread replays its chunk from its exact start.  a > 64, a == 1 or a carried state outside
// int16: one thread does the whole row.  Then low_pass_real in closed form, one thread per output.
//   audio: per channel {avg, now_lpr, prev_lpr_index} in, same out.  y: scratch row per channel (de-emphasised samples
//   when a resampler follows, else unused); out rows: in place (no resampler) or compacted to J samples per channel.
template <bool EVEN, bool D24>
__global__ __launch_bounds__(256) void k_ch_audio(
	int16_t *__restrict__ rows, u64 row_stride, u64 W, int deemph, int a, unsigned magic, int bias, int warm, int serial,
	int fast, int slow, u64 J, const int *__restrict__ audio_in, int *__restrict__ audio_out, int16_t *__restrict__ y_rows, u64 y_stride)
{
	__shared__ uint4 tab[256];
	__shared__ int start[256];
	const int tid = threadIdx.x;
	const u64 c = blockIdx.x;
	int16_t *row = rows + c * row_stride;
	int16_t *yrow = slow > 0 ? y_rows + c * y_stride : row;      // where the (de-emphasised) samples go before resampling
	const int avg_in = audio_in[3 * c];
	// rows that start on a 16-byte boundary are walked eight samples per load (a channel's row starts wherever its stride puts it)
	const bool vec = (((size_t)row | (size_t)yrow) & 15u) == 0;
	if (deemph) {
		const int h = a / 2, xoff = h + bias * a;
		// chunks of at least `warm` samples, multiples of 8, so that every chunk but the first has its warm-up inside the row
		u64 chunk = (W + 255) / 256;
		if (chunk < (u64)warm) chunk = (u64)warm;
		chunk = (chunk + 7) & ~(u64)7;
		const int active = serial ? 1 : (int)((W + chunk - 1) / chunk);
		if (serial) chunk = W;
		const u64 b = (u64)tid * chunk, e = min(W, b + chunk);
		if (tid < active && !serial) {
			int lo, hi;
			if (tid == 0) {
				lo = hi = avg_in;
			} else {
				lo = -32768; hi = 32767;
				if (vec) {
					// eight samples per load, the next eight on their way (b and warm are multiples of 8): a chain step is five instructions, a
					// load's latency hundreds of cycles -- sample by sample this kernel ran at the speed of its loads
					uint4 cur = *reinterpret_cast<const uint4 *>(&row[b - (u64)warm]);
					for (u64 i = b - (u64)warm; i < b; i += 8) {
						const uint4 nxt = *reinterpret_cast<const uint4 *>(&row[i + 8 < b ? i + 8 : i]);
						const uint32_t ww[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
						for (int q = 0; q < 8; q++) {
							const int x = (q & 1) ? hi16(ww[q >> 1]) : lo16(ww[q >> 1]);
							lo = deemph_step_d<EVEN, D24>(lo, x + xoff, x, magic, bias);
							hi = deemph_step_d<EVEN, D24>(hi, x + xoff, x, magic, bias);
						}
						cur = nxt;
					}
				} else {
					for (u64 i = b - (u64)warm; i < b; i++) {
						const int x = row[i];
						lo = deemph_step_d<EVEN, D24>(lo, x + xoff, x, magic, bias);
						hi = deemph_step_d<EVEN, D24>(hi, x + xoff, x, magic, bias);
					}
				}
			}
			int gap = hi - lo;
			if (gap > 63) gap = 63;                               // excluded by `warm`
			const int lo_start = lo;
			int cnt = gap + 1;
			u64 mask = (((u64)1 << gap) - 1);
			u64 i = b;
			if (vec && i + 8 <= e) {
				uint4 cur = *reinterpret_cast<const uint4 *>(&row[i]);
				for (; i + 8 <= e; i += 8) {
					const uint4 nxt = *reinterpret_cast<const uint4 *>(&row[i + 16 <= e ? i + 8 : i]);
					const uint32_t ww[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
					for (int q = 0; q < 8; q++)
						deemph_track<EVEN, D24>(lo, cnt, mask, (q & 1) ? hi16(ww[q >> 1]) : lo16(ww[q >> 1]), a, xoff, magic, bias);
					cur = nxt;
				}
			}
			for (; i < e; i++)
				deemph_track<EVEN, D24>(lo, cnt, mask, (int)row[i], a, xoff, magic, bias);
			tab[tid] = make_uint4((uint32_t)lo_start, ((uint32_t)lo & 0xffffu) | ((uint32_t)gap << 16), (uint32_t)mask, (uint32_t)(mask >> 32));
		}
		__syncthreads();
		if (tid == 0) {
			int s = avg_in;
			if (!serial)
				for (int t = 0; t < active; t++) {
					start[t] = s;
					s = ctab_apply(tab[t], s);
				}
			else
				start[0] = s;
			if (!serial)
				audio_out[3 * c] = s;
		}
		__syncthreads();
		if (tid < active) {
			int s = start[tid];
			if (!serial) {
				u64 i = b;
				if (vec && i + 8 <= e) {
					uint4 cur = *reinterpret_cast<const uint4 *>(&row[i]);
					for (; i + 8 <= e; i += 8) {
						const uint4 nxt = *reinterpret_cast<const uint4 *>(&row[i + 16 <= e ? i + 8 : i]);
						const uint32_t ww[4] = {cur.x, cur.y, cur.z, cur.w};
						uint32_t yy[4];
#pragma unroll
						for (int q = 0; q < 4; q++) {
							const int x0 = lo16(ww[q]), x1 = hi16(ww[q]);
							s = deemph_step_d<EVEN, D24>(s, x0 + xoff, x0, magic, bias);
							const int y0 = s;
							s = deemph_step_d<EVEN, D24>(s, x1 + xoff, x1, magic, bias);
							yy[q] = pack_iq(y0, s);
						}
						*reinterpret_cast<uint4 *>(&yrow[i]) = make_uint4(yy[0], yy[1], yy[2], yy[3]);
						cur = nxt;
					}
				}
				for (; i < e; i++) {
					const int x = row[i];
					s = deemph_step_d<EVEN, D24>(s, x + xoff, x, magic, bias);
					yrow[i] = (int16_t)s;
				}
			} else {
				for (u64 i = b; i < e; i++) {                 // any a, any state: the reference's own expression
					const int d = (int)row[i] - s;
					s += d > 0 ? (d + h) / a : (d - h) / a;
					yrow[i] = (int16_t)s;
				}
				audio_out[3 * c] = s;
			}
		}
		__syncthreads();
	} else {
		if (slow > 0)
			for (u64 i = tid; i < W; i += 256)
				yrow[i] = row[i];
		if (tid == 0)
			audio_out[3 * c] = avg_in;
		__syncthreads();
	}
	if (slow > 0) {
		const u64 p0 = (u64)audio_in[3 * c + 2];
		const int ratio = fast / slow;
		// four outputs per turn, the first four samples of each window requested before any is summed (a window has fast / slow or one more)
		for (u64 j0 = tid; j0 < J; j0 += 4 * 256) {
			u64 wb[4], we[4];
			int pre[4][4];
#pragma unroll
			for (int q = 0; q < 4; q++) {
				const u64 j = j0 + (u64)q * 256;
				const u64 jj = j < J ? j : J - 1;
				wb[q] = jj ? lpr_end(jj - 1, fast, slow, p0) : 0;
				we[q] = lpr_end(jj, fast, slow, p0);
#pragma unroll
				for (int t = 0; t < 4; t++)
					pre[q][t] = yrow[wb[q] + t < W ? wb[q] + t : W - 1];
			}
#pragma unroll
			for (int q = 0; q < 4; q++) {
				const u64 j = j0 + (u64)q * 256;
				if (j >= J)
					break;
				int sum = j ? 0 : audio_in[3 * c + 1];
#pragma unroll
				for (int t = 0; t < 4; t++)
					sum += wb[q] + t < we[q] ? pre[q][t] : 0;
				for (u64 i = wb[q] + 4; i < we[q]; i++)
					sum += yrow[i];
				row[j] = (int16_t)(sum / ratio);
			}
		}
		if (tid == 0) {
			const u64 wb = J ? lpr_end(J - 1, fast, slow, p0) : 0;
			int sum = J ? 0 : audio_in[3 * c + 1];
			for (u64 i = wb; i < W; i++)
				sum += yrow[i];
			audio_out[3 * c + 1] = sum;
			audio_out[3 * c + 2] = (int)(p0 + W * (u64)slow - J * (u64)fast);
		}
	} else if (tid == 0) {
		audio_out[3 * c + 1] = audio_in[3 * c + 1];
		audio_out[3 * c + 2] = audio_in[3 * c + 2];
	}
}

// The same stages over a (segment, channel) grid -- k_ch_audio gives a channel ONE workgroup, i.e. one wave per SIMD on 256 CUs walking
// dependent chains of a thousand steps: 400 us per 1 GiB capture with both stages on.  Here a channel's row is cut into chunks of >= `warm`
// samples, 256 of them per workgroup (a segment), and the chunk tables of a row are composed in a second level as the rx_fm tree does:
//   k_cha_track   grid (segments, channels): per thread one chunk -- warm-up on the two extreme trajectories (chunk 0: the carried state),
//                 lowest candidate + merge mask through the chunk -> a 16-byte table in HBM
//   k_cha_walk    grid (channels), one wave per segment: the lanes are the (at most 64) candidate start states of the segment's first chunk,
//                 each walks the segment's tables (keeping its state in front of every 32nd); one thread chains the segments from the carried
//                 state; eight lanes per segment then walk 32 tables each from the true candidate's checkpoints -> every chunk's start state
//   k_cha_replay  grid (segments, channels): every thread replays its chunk from its exact start -> the de-emphasised row (another buffer than the demodulated one)
//                 and, with a resampler behind, runs low_pass_real inline on the filtered samples (k_cha_replay_rs): they never go to HBM
#define CHA_MAX_SEG 8

// A lane walks ITS chunk, so a wave's loads land on 64 different cache lines.  First form (16 bytes per lane and turn): every line crossed eight
// times (2048 workgroups' working set fits no cache), 160 + 213 us.  Now a lane takes a whole 128-byte line per turn, eight loads back to back
// (cha_load): every line crosses once -- for the READS that is all there is to gain (fetching the wave's 64 lines as whole lines, eight lanes
// to a line, and handing them over through LDS left k_cha_track at 47 us and cost k_cha_replay_rs its occupancy: measured, taken out again).
// The de-emphasised lines that go BACK to HBM are another matter: written lane by lane they are partial-line writes; k_cha_replay sends them
// through 9 KiB of wave-private LDS (rows of 128 + 16 bytes) and stores whole lines, eight lanes to a line: 100 -> 44 us.
struct cha_line { uint4 u[8]; };
__device__ __forceinline__ cha_line cha_load(const int16_t *p)
{
	cha_line l;
#pragma unroll
	for (int k = 0; k < 8; k++)
		l.u[k] = reinterpret_cast<const uint4 *>(p)[k];
	return l;
}
__device__ __forceinline__ int cha_sample(const cha_line &l, int q)        // q: compile-time after unrolling
{
	const uint4 u = l.u[q >> 3];
	const uint32_t w = ((q >> 1) & 3) == 0 ? u.x : ((q >> 1) & 3) == 1 ? u.y : ((q >> 1) & 3) == 2 ? u.z : u.w;
	return (q & 1) ? hi16(w) : lo16(w);
}
#define CHA_ROW_U4 9                                          // a lane's row of the stage in uint4 units: its line + 16 bytes of pad
#define CHA_STAGE_U4 (64 * CHA_ROW_U4)                        // per wave

__device__ __forceinline__ void cha_wave_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// samples [off, off + 64) of the chunk of EVERY lane of the wave (off relative to the chunk's first sample, a multiple of 8; negative: the warm-up
// in front of it): instruction m brings the lines of lanes 8m .. 8m + 7, lane L the 16-byte piece L % 8 of lane 8m + L / 8's line.  Pieces outside the
// row (a wave past the last chunk, the warm-up of the row's first chunk) come as zeros and are never walked.
__device__ __forceinline__ cha_line cha_fetch(const int16_t *__restrict__ row, u64 W, unsigned g_wave, unsigned chunk, unsigned n_chunks, long long off, unsigned lane)
{
	cha_line f;
#pragma unroll
	for (int m = 0; m < 8; m++) {
		const unsigned g = g_wave + 8u * m + (lane >> 3);
		const long long sidx = (long long)g * chunk + off + (long long)(lane & 7u) * 8;
		const bool ok = g < n_chunks && sidx >= 0 && (u64)sidx + 8 <= W;
		f.u[m] = ok ? *reinterpret_cast<const uint4 *>(row + (ok ? sidx : 0)) : make_uint4(0u, 0u, 0u, 0u);
	}
	return f;
}
// fetched pieces -> every lane's own line
__device__ __forceinline__ cha_line cha_hand_over(uint4 *stage, const cha_line &f, unsigned lane)
{
	cha_wave_sync();                                              // the readers of the turn before are done with the stage
#pragma unroll
	for (int m = 0; m < 8; m++)
		stage[(8u * m + (lane >> 3)) * CHA_ROW_U4 + (lane & 7u)] = f.u[m];
	cha_wave_sync();
	cha_line l;
#pragma unroll
	for (int q = 0; q < 8; q++)
		l.u[q] = stage[lane * CHA_ROW_U4 + q];
	return l;
}

template <bool EVEN, bool D24>
__global__ __launch_bounds__(256) void k_cha_track(const int16_t *__restrict__ rows, u64 row_stride, u64 W, int a, unsigned magic, int bias, int warm,
                                                   unsigned chunk, unsigned n_chunks, const int *__restrict__ audio_in, uint4 *__restrict__ ctab)
{
	const unsigned g = blockIdx.x * 256u + threadIdx.x;
	if (g >= n_chunks)
		return;
	const u64 c = blockIdx.y;
	const int16_t *row = rows + c * row_stride;
	const bool vec = ((size_t)row & 15u) == 0;
	const int h = a / 2, xoff = h + bias * a;
	const u64 b = (u64)g * chunk, e = min(W, b + chunk);
	int lo, hi;
	if (g == 0) {
		lo = hi = audio_in[3 * c];
	} else {
		lo = -32768; hi = 32767;
		u64 i = b - (u64)warm;
		if (vec && i + 64 <= b) {
			cha_line cur = cha_load(&row[i]);
			for (; i + 64 <= b; i += 64) {
				const cha_line nxt = cha_load(&row[i + 128 <= b ? i + 64 : i]);
#pragma unroll
				for (int q = 0; q < 64; q++) {
					const int x = cha_sample(cur, q);
					lo = deemph_step_d<EVEN, D24>(lo, x + xoff, x, magic, bias);
					hi = deemph_step_d<EVEN, D24>(hi, x + xoff, x, magic, bias);
				}
				cur = nxt;
			}
		}
		for (; i < b; i++) {
			const int x = row[i];
			lo = deemph_step_d<EVEN, D24>(lo, x + xoff, x, magic, bias);
			hi = deemph_step_d<EVEN, D24>(hi, x + xoff, x, magic, bias);
		}
	}
	int gap = hi - lo;
	if (gap > 63) gap = 63;                                       // excluded by `warm`
	const int lo_start = lo;
	int cnt = gap + 1;
	u64 mask = (((u64)1 << gap) - 1);
	u64 i = b;
	if (vec && i + 64 <= e) {
		cha_line cur = cha_load(&row[i]);
		for (; i + 64 <= e; i += 64) {
			const cha_line nxt = cha_load(&row[i + 128 <= e ? i + 64 : i]);
#pragma unroll
			for (int q = 0; q < 64; q++)
				deemph_track<EVEN, D24>(lo, cnt, mask, cha_sample(cur, q), a, xoff, magic, bias);
			cur = nxt;
		}
	}
	for (; i < e; i++)
		deemph_track<EVEN, D24>(lo, cnt, mask, (int)row[i], a, xoff, magic, bias);
	ctab[c * n_chunks + g] = make_uint4((uint32_t)lo_start, ((uint32_t)lo & 0xffffu) | ((uint32_t)gap << 16), (uint32_t)mask, (uint32_t)(mask >> 32));
}

__global__ __launch_bounds__(64 * CHA_MAX_SEG) void k_cha_walk(const uint4 *__restrict__ ctab, unsigned n_chunks, const int *__restrict__ audio_in,
                                                                int *__restrict__ audio_out, int *__restrict__ chunk_start)
{
	extern __shared__ __attribute__((aligned(16))) uint4 cha_tab[];      // the channel's n_chunks tables, then n_chunks ints (the chunk starts)
	__shared__ int ckpt[CHA_MAX_SEG][9][64];                             // every candidate's state in front of chunks 0, 32, .. 224 of its segment, and behind the last
	__shared__ int seg_idx[CHA_MAX_SEG];
	const u64 c = blockIdx.x;
	const unsigned n_seg = (n_chunks + 255) / 256;
	for (unsigned i = threadIdx.x; i < n_chunks; i += blockDim.x)
		cha_tab[i] = ctab[c * n_chunks + i];
	__syncthreads();
	const unsigned sgm = threadIdx.x >> 6, k = threadIdx.x & 63;
	const unsigned g0 = sgm * 256u, g1 = sgm < n_seg ? min(n_chunks, g0 + 256u) : g0;
	if (sgm < n_seg) {
		const uint4 t0 = cha_tab[g0];
		const int gap = (int)(t0.y >> 16);
		int v = (int)t0.x + min((int)k, gap);                        // lanes beyond the candidates repeat the last one
		// four tables requested ahead of the dependent chain (an LDS read's latency is most of a step otherwise)
		unsigned g = g0;
		for (; g + 4 <= g1; g += 4) {
			if (((g - g0) & 31u) == 0)
				ckpt[sgm][(g - g0) >> 5][k] = v;
			const uint4 ta = cha_tab[g], tb = cha_tab[g + 1], tc = cha_tab[g + 2], td = cha_tab[g + 3];
			v = ctab_apply(ta, v); v = ctab_apply(tb, v); v = ctab_apply(tc, v); v = ctab_apply(td, v);
		}
		for (; g < g1; g++) {
			if (((g - g0) & 31u) == 0)
				ckpt[sgm][(g - g0) >> 5][k] = v;
			v = ctab_apply(cha_tab[g], v);
		}
		ckpt[sgm][8][k] = v;                                         // the segment's end state for this candidate
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		int v = audio_in[3 * c];
		for (unsigned sg = 0; sg < n_seg; sg++) {
			const uint4 t0 = cha_tab[sg * 256u];
			int idx = v - (int)t0.x;
			const int gap = (int)(t0.y >> 16);
			idx = idx < 0 ? 0 : (idx > gap ? gap : idx);              // inside [0, gap] by the warm-up's guarantee
			seg_idx[sg] = idx;
			v = ckpt[sg][8][idx];
		}
		audio_out[3 * c] = v;
	}
	__syncthreads();
	// every chunk's exact start state: the replay kernels begin without a serial walk of their own (a workgroup's thread 0 walking 256 tables
	// held its other 255 threads for ten microseconds, four rounds of workgroups per CU).  The segment's true candidate is known now, and its
	// state in front of every 32nd chunk was kept: eight lanes per segment walk 32 tables each
	int *const st = reinterpret_cast<int *>(cha_tab + n_chunks);       // [n_chunks] behind the tables: the starts leave coalesced
	if (sgm < n_seg && k < 8) {
		unsigned g = g0 + 32u * k;
		const unsigned ge = min(g1, g + 32u);
		if (g < ge) {
			int v = ckpt[sgm][k][seg_idx[sgm]];
			for (; g + 4 <= ge; g += 4) {
				const uint4 ta = cha_tab[g], tb = cha_tab[g + 1], tc = cha_tab[g + 2], td = cha_tab[g + 3];
				st[g] = v; v = ctab_apply(ta, v);
				st[g + 1] = v; v = ctab_apply(tb, v);
				st[g + 2] = v; v = ctab_apply(tc, v);
				st[g + 3] = v; v = ctab_apply(td, v);
			}
			for (; g < ge; g++) {
				st[g] = v;
				v = ctab_apply(cha_tab[g], v);
			}
		}
	}
	__syncthreads();
	for (unsigned i = threadIdx.x; i < n_chunks; i += blockDim.x)
		chunk_start[c * n_chunks + i] = st[i];
}

// de-emphasis only: every thread replays its chunk from its exact start, in -> out (two buffers: the demodulated rows stay as they are); the
// filtered lines go back through the stage and leave as whole lines, eight lanes to a line
template <bool EVEN, bool D24>
__global__ __launch_bounds__(256) void k_cha_replay(const int16_t *__restrict__ rows, u64 row_stride, u64 W, int a, unsigned magic, int bias,
                                                    unsigned chunk, unsigned n_chunks, const int *__restrict__ chunk_start,
                                                    const int *__restrict__ audio_in, int *__restrict__ audio_out, int16_t *__restrict__ y_rows, u64 y_stride)
{
	__shared__ __attribute__((aligned(16))) uint4 cha_stage[4 * CHA_STAGE_U4];
	const unsigned lane = threadIdx.x & 63u, g_wave = blockIdx.x * 256u + (threadIdx.x & ~63u), g = g_wave + lane;
	if (g_wave >= n_chunks)
		return;
	uint4 *const stage = cha_stage + (threadIdx.x >> 6) * CHA_STAGE_U4;
	const bool valid = g < n_chunks;
	const u64 c = blockIdx.y;
	const int16_t *row = rows + c * row_stride;
	int16_t *yrow = y_rows + c * y_stride;
	const bool staged = (((size_t)row | (size_t)yrow) & 15u) == 0 && (chunk & 63u) == 0;
	int v = valid ? chunk_start[c * n_chunks + g] : 0;
	if (g == 0) {                                                 // the resampler's carries pass through
		audio_out[3 * c + 1] = audio_in[3 * c + 1];
		audio_out[3 * c + 2] = audio_in[3 * c + 2];
	}
	const int h = a / 2, xoff = h + bias * a;
	const u64 b = (u64)g * chunk, e = valid ? min(W, b + chunk) : b;
	const int nturn = staged ? (int)(chunk / 64u) : 0;
	u64 i = b;
	cha_line f;
	if (staged)
		f = cha_fetch(row, W, g_wave, chunk, n_chunks, 0, lane);
	for (int t = 0; t < nturn; t++) {
		const cha_line cur = cha_hand_over(stage, f, lane);
		if (t + 1 < nturn)
			f = cha_fetch(row, W, g_wave, chunk, n_chunks, 64ll * (t + 1), lane);
		// the filtered samples go into the lane's OWN row of the stage, sixteen bytes at a time, over the input line it has just taken out of it
		// (LDS operations of a wave retire in order; nobody else reads that row before the barrier below)
		if (i + 64 <= e) {
#pragma unroll
			for (int q = 0; q < 8; q++) {
				uint32_t yy[4];
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const int x0 = cha_sample(cur, 8 * q + 2 * k), x1 = cha_sample(cur, 8 * q + 2 * k + 1);
					v = deemph_step_d<EVEN, D24>(v, x0 + xoff, x0, magic, bias);
					const int y0 = v;
					v = deemph_step_d<EVEN, D24>(v, x1 + xoff, x1, magic, bias);
					yy[k] = pack_iq(y0, v);
				}
				stage[lane * CHA_ROW_U4 + q] = make_uint4(yy[0], yy[1], yy[2], yy[3]);
			}
			i += 64;
		}
		cha_wave_sync();
#pragma unroll
		for (int m = 0; m < 8; m++) {
			const unsigned r = 8u * m + (lane >> 3), gr = g_wave + r;
			const u64 br = (u64)gr * chunk, er = gr < n_chunks ? min(W, br + chunk) : br;
			if (br + 64ull * (u64)t + 64 <= er)                    // lane r walked this turn
				*reinterpret_cast<uint4 *>(yrow + br + 64ull * (u64)t + (lane & 7u) * 8u) = stage[r * CHA_ROW_U4 + (lane & 7u)];
		}
	}
	for (; i < e; i++) {
		const int x = row[i];
		v = deemph_step_d<EVEN, D24>(v, x + xoff, x, magic, bias);
		yrow[i] = (int16_t)v;
	}
}

// de-emphasis replay with low_pass_real (rtl_fm.c:389-409) run INLINE on the filtered samples -- they never go to HBM.  The resampler's phase
// before sample x is (p0 + x slow) mod fast and floor((p0 + x slow) / fast) outputs exist by then: a thread starts from those two numbers, owns
// the windows that START in its chunk (the one in progress at its first sample is the left neighbour's, unless the sample in front emitted:
// phase < slow) and walks on past its chunk to finish its last one.  The workgroup's outputs are a contiguous range: staged in LDS as int16, they
// leave coalesced.  The thread that reaches the end of the row inside a window it owns leaves the carries (now_lpr, prev_lpr_index).
template <bool EVEN, bool D24>
__global__ __launch_bounds__(256) void k_cha_replay_rs(const int16_t *__restrict__ rows, u64 row_stride, u64 W, int a, unsigned magic, int bias,
                                                       unsigned chunk, unsigned n_chunks, const int *__restrict__ chunk_start,
                                                       int fast, int slow, int ratio, float rinv, const int *__restrict__ audio_in, int *__restrict__ audio_out,
                                                       int16_t *__restrict__ out_rows, u64 out_stride, unsigned cap)
{
	extern __shared__ __attribute__((aligned(16))) int16_t cha_out[];      // [cap] the workgroup's outputs
	const unsigned tid = threadIdx.x, g = blockIdx.x * 256u + tid;
	const u64 c = blockIdx.y;
	const int16_t *row = rows + c * row_stride;
	const bool vec = ((size_t)row & 15u) == 0;
	const unsigned active = min(256u, n_chunks - blockIdx.x * 256u);
	int v = tid < active ? chunk_start[c * n_chunks + g] : 0;
	const u64 p0 = (u64)audio_in[3 * c + 2];
	// first output of the workgroup: windows that started before its first sample b_wg: the emissions so far, + 1 unless the sample in front emitted
	const u64 b_wg = (u64)blockIdx.x * 256u * chunk, e_wg = min(W, b_wg + 256ull * chunk);
	const u64 t_wg = p0 + b_wg * (u64)slow, t_we = p0 + e_wg * (u64)slow;
	const u64 J0 = b_wg ? t_wg / (u64)fast + ((t_wg % (u64)fast) < (u64)slow ? 0u : 1u) : 0u;
	const u64 J1 = e_wg < W ? t_we / (u64)fast + ((t_we % (u64)fast) < (u64)slow ? 0u : 1u) : t_we / (u64)fast;   // the row's last window stays unfinished
	if (tid < active) {
		const int h = a / 2, xoff = h + bias * a;
		const u64 b = (u64)g * chunk, e = min(W, b + chunk);
		const u64 t_b = p0 + b * (u64)slow;
		unsigned j = (unsigned)(t_b / (u64)fast - J0);                   // index (in the staging) of the window in progress at b ...
		int p = (int)(t_b % (u64)fast);                                 // ... and the phase in front of sample b
		bool own = g == 0 || p < slow;
		int sum = g == 0 ? audio_in[3 * c + 1] : 0;
		bool first = g == 0;                                            // the carried partial sum may be anything: exact division for output 0
		u64 i = b;
		// one sample: de-emphasis, accumulate, phase; an emission stores (int16)(sum / ratio) -- C's truncating division, by the reciprocal rounded
		// up where that is exact (ratio <= 32, |sum| <= 33 * 32768: every window but one that starts with the carried sum)
#define CHA_RS_STEP(X) do { \
			const int x_ = (X); \
			v = deemph_step_d<EVEN, D24>(v, x_ + xoff, x_, magic, bias); \
			sum += v; p += slow; \
			if (p >= fast) { \
				p -= fast; \
				if (own) cha_out[j] = (int16_t)((first || rinv == 0.0f) ? sum / ratio : (int)((float)sum * rinv)); \
				j++; sum = 0; own = true; first = false; \
			} } while (0)
		if (vec && i + 64 <= e) {
			cha_line cur = cha_load(&row[i]);
			for (; i + 64 <= e; i += 64) {
				const cha_line nxt = cha_load(&row[i + 128 <= e ? i + 64 : i]);
#pragma unroll
				for (int q = 0; q < 64; q++)
					CHA_RS_STEP(cha_sample(cur, q));
				cur = nxt;
			}
		}
		for (; i < e; i++)
			CHA_RS_STEP((int)row[i]);
		// past the chunk: the window in progress is this thread's to finish (a sample whose predecessor emitted starts the neighbour's)
		for (; i < W && p >= slow; i++)
			CHA_RS_STEP((int)row[i]);
#undef CHA_RS_STEP
		if (i == W && own) {
			audio_out[3 * c + 1] = sum;
			audio_out[3 * c + 2] = p;
		}
	}
	__syncthreads();
	const unsigned cnt = (unsigned)(J1 - J0);
	int16_t *dst = out_rows + c * out_stride + J0;
	for (unsigned k = tid; k < cnt && k < cap; k += 256)
		dst[k] = cha_out[k];
}
