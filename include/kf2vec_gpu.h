/*
 * kf2vec_gpu.h -- C-ABI of the MI355X (gfx950) k-mer frequency-vector builder.
 *
 * Drop-in boundary for kf2vec's `get_frequencies` hot path
 * (reference kf2vec/main.py:250-373).  The reference crosses a PROCESS boundary
 * there: it runs the external C++ counter Jellyfish twice per genome
 *     jellyfish count -m K -s 100M -t P -C <in> -o <x>.jf     (main.py:309-311)
 *     jellyfish dump -c <x>.jf_0 > <x>.dump                    (main.py:317-319)
 * then pandas-joins the dump onto the sorted canonical vocabulary
 * (main.py:278-296, 323-328), normalises (332-342) and formats one `.kf` line
 * (344-357).  This library replaces all of that with device kernels plus a
 * host formatter; the Python host (kf2vecfsw_amd/) binds it with ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; `d_` pointers are device (HBM) pointers,
 *     e.g. `torch.Tensor.data_ptr()` of a ROCm tensor; the CALLER owns every buffer;
 *   - `stream` is a hipStream_t (NULL = default stream); device entry points only
 *     enqueue work, so they can be graph-captured -- with one exception:
 *     kf_count_batch at k >= 10 allocates the library's workspace on first use
 *     and grows its piece table (a device sync) when n_genomes exceeds every
 *     earlier call; kf_workspace_reserve() does both up front;
 *   - return 0 on success, a negative KF_E* code on failure; the message is in
 *     kf_last_error() (thread-local).  Errors are never silent (deliberate
 *     deviation from main.py:309-311, which discards Jellyfish's stderr/status).
 *
 * Internal 2-bit base code ("kf code"): A=0 C=1 T=2 G=3, i.e. ((ascii >> 1) & 3)
 * for ACGTacgt; complement = code ^ 2.  A k-mer code has its first base in the
 * most significant pair.  Columns (bins) are the rank of the canonical k-mer in
 * the lexicographically sorted canonical vocabulary -- the order of the
 * reference's vocab files (kf2vec/data/) and hence of every `.kf` line.
 */
#ifndef KF2VEC_GPU_H
#define KF2VEC_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KF_ABI_VERSION 1

#define KF_OK 0
#define KF_EINVAL (-1)   /* bad argument (k out of range, null pointer, ...) */
#define KF_EHIP (-2)     /* HIP runtime error */
#define KF_ERANGE (-3)   /* output buffer too small / size overflow */
#define KF_EFORMAT (-4)  /* unparseable input */

#define KF_MIN_K 2
#define KF_MAX_K 12      /* dense device kernels; the CLI accepts 3..11 */
#define KF_SPARSE_MAX_K 31  /* kf_sparse_count (get_kmers, main.py:81-82) */

/* kf_count_batch and kf_rows_accumulate flags */
#define KF_ACCUMULATE 1u /* do not zero d_counts / d_totals first; add into the destination rows */

/* input formats */
#define KF_FMT_AUTO 0    /* sniff: first byte '@' -> FASTQ, else FASTA */
#define KF_FMT_FASTA 1
#define KF_FMT_FASTQ 2

int kf_abi_version(void);
const char* kf_last_error(void);

/* Number of bins (= lines of the reference vocab file for k, main.py:278-296):
 * 4^k/2 for odd k, (4^k + 4^(k/2))/2 for even k.  0 if k is out of range. */
uint64_t kf_num_bins(int k);

/* Bin tables for k (replaces the vocab file read, main.py:278-296, and the
 * dump->vocab left-merge, main.py:323-328):
 *   code2col[4^k] : kf code of ANY k-mer -> column of its canonical class
 *   col2rep[nbins]: column -> the kf code the device kernels count it under
 *                   (min(code, revcomp(code)) in kf-code order)
 * Either pointer may be NULL.  *nbins receives kf_num_bins(k). */
int kf_tables(int k, uint32_t* code2col, uint32_t* col2rep, uint64_t* nbins);

/* Sorted canonical vocabulary as text, "KMER\n" per line (byte-identical to the
 * reference's kf2vec/data files for k=3..9).  cap >= nbins*(k+1). */
int kf_vocab_text(int k, char* out, uint64_t cap, uint64_t* written);

/* Record index of one FASTA/FASTQ buffer: the byte ranges that are NOT sequence
 * (FASTA header lines; FASTQ '@' header, '+' and quality lines), as sorted,
 * disjoint [start, end) pairs offset by `base` (the buffer's position inside the
 * device batch).  Newlines between sequence lines are not excluded: the device
 * kernel skips them, so k-mers span line breaks but never records.
 * out_iv holds cap_pairs pairs; on KF_ERANGE *n_pairs is the count needed. */
int kf_index_records(const uint8_t* bytes, uint64_t len, int fmt, uint64_t base,
                     uint64_t* out_iv, uint64_t cap_pairs, uint64_t* n_pairs,
                     int* fmt_detected);

/* Read n files into one host buffer (replaces the per-file open/read that the
 * reference leaves to Jellyfish, main.py:309-311): file i (sizes[i] bytes,
 * checked against the file) goes to dst + off[i], and the bytes
 * [off[i] + sizes[i], off[i+1]) are set to '\n' (transparent padding).  The reads
 * are cut into pieces of at most `piece` bytes (pread) shared by n_threads native
 * threads, so a few large files still keep every thread reading; no Python (or
 * its interpreter lock) runs per piece.  KF_EINVAL on an unreadable or
 * resized file (the message names it). */
int kf_read_files(const char* const* paths, int32_t n, const uint64_t* sizes, const uint64_t* off,
                  uint8_t* dst, uint64_t piece, int n_threads);

/* The FASTA record index of a batch resident in HBM (what kf_index_records finds
 * per file, found on the device so the host only copies the files): the header
 * lines -- a line starting with '>' at a genome start or after '\n', up to its
 * '\n' or the genome end -- as sorted [start, end) pairs d_excl[2i], d_excl[2i+1]
 * (absolute positions; adjacent header lines stay separate pairs, which the
 * count kernels treat alike).  *d_n_pairs (device) receives the number of
 * header lines; only the first cap_pairs are written, so a caller reads it back
 * and runs again with a larger table if it was exceeded.  batch_bytes = goff[n];
 * d_scratch >= ceil(batch_bytes / 4096) + 1 words.  FASTA only (a FASTQ batch
 * goes to kf_index_fastq).  Asynchronous on `stream`. */
int kf_index_fasta(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_genomes,
                   uint64_t batch_bytes, uint64_t* d_excl, uint64_t cap_pairs,
                   uint64_t* d_n_pairs, uint32_t* d_scratch, uint64_t scratch_words, void* stream);

/* The FASTQ record index of a batch resident in HBM: every genome of a batch
 * laid out as for kf_count_batch (d_bytes 16-byte aligned and readable up to
 * batch_bytes = goff[n] rounded up to 16) is read as FASTQ in the regular
 * four-line form.  With j the 0-based number of a line inside its genome (lines
 * end at '\n' only, a genome's first line starts at goff[g]) and L its length
 * without the '\n' ('\r' counts), a genome is REGULAR if for every line up to
 * its last non-empty one
 *   j % 4 == 0: L > 0 and the line starts with '@';
 *   j % 4 == 1: the line is empty or does not start with '+';
 *   j % 4 == 2: L > 0 and the line starts with '+';
 *   j % 4 == 3: L >= L(line j - 2), and the line is empty if line j - 2 is.
 * Trailing empty lines (the '\n' padding included), a genome that stops in the
 * middle of a record and one without a final '\n' stay regular.  For a regular
 * genome the excluded bytes of kf_index_records(KF_FMT_FASTQ) are the bytes of
 * every line with j % 4 != 1, and this call writes them as sorted, disjoint,
 * non-empty [start, end) pairs d_excl[2i], d_excl[2i+1] (absolute positions,
 * the form kf_count_batch takes): one pair for the genome's first header line,
 * then one per record that has a '+' line, from the start of that line to the
 * end of the next record's header line (or of the genome's last non-empty
 * line) -- records + 1 pairs for a genome of whole records, none for a genome
 * of '\n' only.  No pair crosses goff[g + 1].
 *   d_n[0] (device) : the number of pairs; only the first cap_pairs are written
 *   d_n[1] (device) : the number of '\n' in the batch.  The index works from a
 *                     table of their positions that holds cap_lines entries; if
 *                     d_n[1] > cap_lines nothing else was computed (d_n[0] = 0)
 *   d_status[g]     : 0 = regular; 1 = not regular; 2 = goff[g] > goff[g + 1] or
 *                     goff[g + 1] > batch_bytes (nothing of that genome is read).
 *                     Only genomes all of whose pairs fit below cap_pairs are
 *                     checked.  The pairs of a genome that is not regular are
 *                     unspecified but lie inside its bytes and inside the table.
 * So a caller reads d_n and d_status back once and runs again with larger tables
 * if d_n[1] > cap_lines or d_n[0] > cap_pairs; a batch of d_n[1] newlines and n
 * genomes has at most d_n[1] / 4 + 2 n pairs.  d_scratch (8-byte aligned) holds
 * kf_index_fastq_scratch_bytes(batch_bytes, n_genomes, cap_lines) bytes: 8 per
 * table entry, 8 per 4 KiB block of the batch (plus 1/1024 of that for the
 * scan's upper levels) and about 32 per genome.  Nothing is allocated and no
 * workgroup waits for another: ten launches, the newline counts per 4 KiB block,
 * a three-level scan (1,024 entries per workgroup and level, so batch_bytes <=
 * 4 TiB and n_genomes <= 2^30), the positions, one thread per genome, the same
 * scan over the genomes' pair counts, one thread per pair.  KF_EINVAL for
 * n_genomes < 0, null or misaligned pointers and sizes past those limits,
 * KF_ERANGE for a scratch that is too small -- before anything is launched.
 * Asynchronous on `stream`. */
uint64_t kf_index_fastq_scratch_bytes(uint64_t batch_bytes, int32_t n_genomes, uint64_t cap_lines);
int kf_index_fastq(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_genomes,
                   uint64_t batch_bytes, uint64_t* d_excl, uint64_t cap_pairs, uint64_t cap_lines,
                   uint64_t* d_n, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
                   void* stream);

/* Count canonical k-mers of a batch of genomes already resident in HBM
 * (replaces `jellyfish count -C` + `jellyfish dump -c`, main.py:309-323).
 *   d_bytes    : batch bytes, 16-byte aligned; genome g is
 *                d_bytes[d_goff[g], d_goff[g+1]); the allocation must be readable
 *                up to d_goff[n] rounded up to 16 bytes (vector loads)
 *   d_goff     : n_genomes+1 non-decreasing offsets (device)
 *   d_excl     : 2*n_excl sorted disjoint [start,end) pairs (device) from
 *                kf_index_records, positions absolute in d_bytes (may be NULL if 0)
 *   d_code2col, d_col2rep : kf_tables(k) uploaded to the device
 *   d_counts   : n_genomes x nbins uint32 (column order), zeroed first unless
 *                flags & KF_ACCUMULATE
 *   d_totals   : n_genomes uint64, number of k-mers counted per genome
 * Asynchronous on `stream`.  For k >= 10 the library counts through a device
 * workspace (about 9 GB on a 256-CU device: 2 bytes of sorted records per byte
 * of the 8 MiB genome piece each CU holds, in two slots for the staggered
 * phases) plus a piece table of n_genomes+1 words, kept until
 * kf_workspace_release().  Both are allocated on first use;
 * the piece table is re-allocated behind a hipDeviceSynchronize() when
 * n_genomes exceeds its capacity (it grows at least 2x).  Call
 * kf_workspace_reserve() first to keep every kf_count_batch asynchronous and
 * allocation-free.  Launches on different streams of one device that use the
 * workspace are ordered by the library. */
int kf_count_batch(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_genomes,
                   const uint64_t* d_excl, uint64_t n_excl,
                   const uint32_t* d_code2col, const uint32_t* d_col2rep, int k,
                   uint32_t* d_counts, uint64_t* d_totals, uint32_t flags, void* stream);

/* Column-wise sums of count rows on the device: what adds the rows of a file
 * that get_frequencies counted in pieces (each piece one genome of a
 * kf_count_batch) up into the file's row.  d_src is n_src x nbins uint32 with
 * d_src_totals[n_src]; d_seg holds n_dst + 1 non-decreasing offsets into the
 * source rows (the seg_row0 idiom of kf_write_kf_segments), and destination row
 * r of d_dst (n_dst x nbins) receives the column-wise sum of the source rows
 * [d_seg[r], d_seg[r+1]), d_dst_totals[r] the sum of their totals.
 *   flags = 0             : the row, its total and d_status[r] are overwritten;
 *                           an empty segment gives zeros, total 0, status 0
 *   flags = KF_ACCUMULATE : the sum is added to what the row and its total hold
 *                           and d_status[r] is OR-ed into, so a file's pieces may
 *                           come in several calls; an empty segment leaves the
 *                           row, its total and its status untouched
 *   d_status[r] bit 0     : a column's true sum passed 2^32 - 1.  That column is
 *                           stored as UINT32_MAX (so any later accumulating add
 *                           to it carries again: the flag is sticky); a sum of
 *                           exactly 2^32 - 1 is no overflow.  Errors are never
 *                           silent: a caller reads the status before it uses
 *                           the row.  The u64 totals are not checked.
 *   d_status[r] == 2      : the segment table is bad -- an offset below 0 or
 *                           above n_src, or a decrease.  Checked on the device;
 *                           then nothing of d_dst or d_dst_totals is written and
 *                           every status word is 2.
 * d_dst must not overlap d_src.  Rows are read and written 16 bytes per thread
 * when nbins % 4 == 0 and both matrices are 16-byte aligned (every k >= 3), else
 * 4 bytes.  KF_EINVAL for a null or misaligned pointer, a negative count or
 * nbins == 0, before anything is launched.  One launch (after a memset of the
 * status words without KF_ACCUMULATE): asynchronous on `stream`, no allocation,
 * no workgroup waits for another. */
int kf_rows_accumulate(const uint32_t* d_src, const uint64_t* d_src_totals, int32_t n_src,
                       const int32_t* d_seg, int32_t n_dst, uint64_t nbins,
                       uint32_t* d_dst, uint64_t* d_dst_totals, uint32_t* d_status,
                       uint32_t flags, void* stream);

/* Allocate up front, on the current device, everything kf_count_batch(k, n)
 * needs for any n <= max_genomes: the k >= 10 bucket tables, workspace and
 * piece table, and the kernel attributes of k.  Afterwards such calls neither
 * allocate nor synchronise.  Synchronous; may be called again with a larger
 * max_genomes. */
int kf_workspace_reserve(int k, int32_t max_genomes);

/* Grid the count kernel will use on the current device for k (workgroups,
 * threads per workgroup, dynamic LDS bytes); for roofline accounting.
 * Kernel choice: k <= 7 the pair kernel K1x (k1x_kernel<k>: (k+1)-mer pairs
 * plus single k-mers in LDS), k = 8 its single-pass form (k1x_kernel<8>),
 * k = 9 its byte-counter form (k1x_kernel<9>: all 131,072 canonical classes
 * as u8 LDS counters, carries corrected exactly from the adds' returns), k >= 10
 * the two-phase bucket kernels (bucket_kernel<k>).
 * No environment variable changes the choice in the product library. */
int kf_count_launch_info(int k, int* grid, int* block, int* lds_bytes);

/* ---- get_kmers at any k = 2..31 (replaces `jellyfish count -m K -C` +
 * `jellyfish dump -c -t` of main.py:133-160, which keep the PRESENT canonical
 * k-mers only).  For every genome of a batch laid out as for kf_count_batch:
 * its distinct canonical k-mers in ascending standard 2-bit code (A0 C1 G2 T3,
 * first base most significant: lexicographic order of the k-mer strings, the
 * order of the vocab files) and their counts.  Same input semantics as
 * kf_count_batch.  Genome g's results are d_keys[goff[g] + i] and
 * d_counts[goff[g] + i] for i < d_nuniq[g] (a genome has at most goff[g+1] -
 * goff[g] distinct k-mers, so both arrays hold batch_bytes = goff[n] entries).
 * The device counts each genome's keys per bucket (their top min(10, 2k)
 * bits), scatters every window's key once into its bucket (decoupled
 * look-back per bucket), packs whole buckets into chunks of <= 16,384 keys
 * (12,288 for k <= 16) and
 * sorts each chunk in LDS (10-bit MSD passes plus a fix-up of runs of equal
 * top bits); buckets larger than a chunk are sorted by LSD passes in an
 * overflow area.  Then run-length encoding.  d_work must hold
 * kf_sparse_workspace_bytes(k, batch_bytes, n_genomes) bytes: two key areas of
 * 4 (k <= 16) or 8 B per input byte plus ~1 B per byte of tables, so with the
 * outputs a call needs ~21 (k <= 16) or ~29 device bytes per input byte.  batch_bytes < 2^32 and d_bytes
 * 16-byte aligned (KF_EINVAL otherwise, as kf_count_batch).
 * Asynchronous on `stream`, no allocation, no host synchronisation.  The
 * offsets are checked on the device: if d_goff decreases or d_goff[n] >
 * batch_bytes, nothing is read or written and every d_nuniq[g] is UINT64_MAX.
 * The sorted keys are checked on the device too: a genome whose keys are not
 * in order, or a sort pass whose tile-to-tile prefix exchange (decoupled
 * look-back) stalled past its bound, makes every d_nuniq[g] UINT64_MAX - 1
 * (fail loudly, never silently or by hanging). */
uint64_t kf_sparse_workspace_bytes(int k, uint64_t batch_bytes, int32_t n_genomes);
int kf_sparse_count(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_genomes,
                    uint64_t batch_bytes, const uint64_t* d_excl, uint64_t n_excl, int k,
                    void* d_work, uint64_t work_bytes, uint64_t* d_keys, uint32_t* d_counts,
                    uint64_t* d_nuniq, void* stream);

/* ---- the get_kmers matrix (main.py:147-172) built on the device, from the keys
 * and counts kf_sparse_count leaves there (or the non-zero bins of a
 * kf_count_batch row, as standard codes): float32 rows of k + 1 columns, the k
 * bases of a k-mer as get_kmers digits (A0 T1 C2 G3, main.py:118; first base
 * first) and then its count divided by its genome's divisor.  One call writes
 * the rows [row_lo, row_hi) (the SLAB) of a matrix that n_seg segments (genomes)
 * tile, so a matrix of any size can be produced through a fixed buffer:
 *   d_keys, d_counts : standard codes (A0 C1 G2 T3, first base most significant)
 *                      and counts, u32 (count_bytes = 4) or u64 (8)
 *   d_src0[n_seg]    : index in d_keys / d_counts of segment s's first k-mer
 *   d_n[n_seg]       : the number of k-mers (rows) of segment s; the caller
 *                      vouches that d_src0[s] + d_n[s] entries are readable
 *   d_dst0[n_seg+1]  : the matrix row of segment s's first k-mer, non-decreasing;
 *                      d_dst0[n_seg] is the number of matrix rows
 *   d_denom[n_seg]   : segment s's divisor
 *   d_out            : the slab, 16-byte aligned, (row_hi - row_lo) x (k + 1)
 *                      floats, row-major; its element 0 is (row_lo, column 0)
 * Matrix row d_dst0[s] + i (i < d_n[s]) holds the digits 0.0f .. 3.0f of key
 * d_keys[d_src0[s] + i] and (float)count / d_denom[s]: conversion and division
 * round to nearest even (IEEE), bit-equal to numpy's
 * `c.astype(np.float32) / np.float32(denom)`.  Every other row -- those of
 * [d_dst0[s] + d_n[s], d_dst0[s+1]) and those below d_dst0[0] -- is written as
 * zeros.  So d_dst0 = the exclusive prefix sum of d_n gives the genomes' matrices
 * packed back to back, and d_dst0[s] = s * Nmax a zero-padded [n_seg, Nmax, k+1]
 * batch that needs no memset.  Every float of the slab is written once; nothing
 * outside it is.  The tables are checked on the device: if d_dst0 decreases,
 * d_n[s] > d_dst0[s+1] - d_dst0[s] or row_hi > d_dst0[n_seg], then *d_status = 2
 * and nothing of d_out is written; otherwise *d_status = 0.  KF_EINVAL, before
 * anything is launched, for k outside 2..31, count_bytes not 4 or 8, n_seg < 0,
 * row_lo > row_hi, a null pointer or a misaligned one (8 bytes for the u64
 * arrays, count_bytes for d_counts, 4 for d_denom and d_status, 16 for d_out).
 * n_seg == 0 writes *d_status = 0 and nothing else; an empty slab (row_lo ==
 * row_hi) checks the tables and writes no row.  One launch: asynchronous on
 * `stream`, no allocation, no workgroup waits for another.  The kernel works in
 * tiles of kf_kmers_tile_rows() slab rows (a multiple of 4). */
int kf_kmers_tile_rows(void);
int kf_kmers_rows(const uint64_t* d_keys, const void* d_counts, int count_bytes,
                  const uint64_t* d_src0, const uint64_t* d_n, const uint64_t* d_dst0,
                  const float* d_denom, int32_t n_seg, int k, uint64_t row_lo, uint64_t row_hi,
                  float* d_out, uint32_t* d_status, void* stream);

/* ---- the union of two sorted (key, count) lists on the device: how get_kmers
 * joins the pieces of a FASTA file above 1 GiB (each piece's kf_sparse_count
 * result into the file's running result), with two inputs and one output in
 * memory and no sort.
 *   d_keys_a[n_a], d_keys_b[n_b] : u64 keys, each list STRICTLY ASCENDING in
 *                      unsigned order (what kf_sparse_count leaves per genome)
 *   d_counts_a, d_counts_b : their counts, u32 (count_bytes = 4) or u64 (8),
 *                      chosen per side; n_a and n_b are host values and may be 0
 *   d_keys_out, d_counts_out : n_a + n_b u64 entries each; no overlap with an input
 *   d_n_out          : one u64 on the device, the number of output entries
 * The output is the ascending union of the keys: a key of both lists appears
 * once with the sum of its two counts, a key of one list keeps its count, all
 * counts as u64 (sums are not checked for wrap, like kf_rows_accumulate's
 * totals).  Entries at and past *d_n_out are unspecified; nothing outside
 * [0, n_a + n_b) of either output array is written.
 * The order is checked on the device before anything depends on it: if either
 * list has an adjacent pair that is equal or descending (anywhere: inside a tile
 * of the kernel or across a tile edge), then *d_status = 1, *d_n_out = 0 and the
 * merge kernels return without reading the lists; otherwise *d_status = 0.  For
 * any input contents the call reads and writes only inside the stated arrays.
 * KF_EINVAL, before anything is launched, for count_bytes not 4 or 8, n_a + n_b
 * above 2^34 entries (the limit: one workgroup per tile within 2^32 threads per
 * launch; index arithmetic is 64-bit throughout), a null pointer (the key and
 * count pointers of a list of length 0 may be null) or a misaligned one (8 bytes
 * for the u64 arrays, d_n_out and d_scratch, count_bytes for the counts, 4 for
 * d_status).  KF_ERANGE if scratch_bytes < kf_sparse_merge_scratch_bytes(n_a,
 * n_b) (16 B per tile and a few words; 0 for sizes above the limit).
 * Merge path in tiles of kf_sparse_merge_tile() merged positions (a multiple of
 * 64), one workgroup each: an order check, a count launch, the scan of the
 * tiles' counts, a scatter launch.  Asynchronous on `stream`, no allocation, no
 * host synchronisation, and no workgroup waits for another. */
int      kf_sparse_merge_tile(void);
uint64_t kf_sparse_merge_scratch_bytes(uint64_t n_a, uint64_t n_b);
int kf_sparse_merge(const uint64_t* d_keys_a, const void* d_counts_a, int count_bytes_a, uint64_t n_a,
                    const uint64_t* d_keys_b, const void* d_counts_b, int count_bytes_b, uint64_t n_b,
                    uint64_t* d_keys_out, uint64_t* d_counts_out, uint64_t* d_n_out,
                    uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* ---- the chunk trainer's samples (kf2vec/datasets.py:27-101, Dataset_chunks_2rows:
 * a contiguous run of a genome's window rows summed column-wise, divided by the
 * grand total, times features_scaler) computed on the device from window count
 * rows that stay there, for a whole table of samples per call:
 *   d_counts         : n_rows x nbins counts, row-major; u16 (count_bytes = 2, the
 *                      rows get_chunks keeps) or u32 (4, a kf_count_batch matrix)
 *   d_lo[n_samples], d_n[n_samples] : sample s covers the rows [d_lo[s], d_lo[s] +
 *                      d_n[s]); samples may overlap, repeat and be empty
 *   cap              : counts enter as min(count, cap) (the reference's cap_data
 *                      is 255); UINT32_MAX = no cap
 *   d_out            : n_samples x nbins, float32 (out_bytes = 4) or float64 (8)
 *   d_work           : kf_chunk_features_scratch_bytes(n_samples) bytes (a u64
 *                      total per sample)
 * With c_j = the sum of min(count, cap) over the sample's rows in column j and T
 * = the sum of c_j over all columns, both exact integers (u16 and u32 rows are
 * summed in 64 bits, for any d_n), d_out[s * nbins + j] = (double)c_j / (double)T
 * * scaler in float64, every step rounded to nearest even (integers at or above
 * 2^53 included, as numpy's astype(float64) rounds them), and rounded once more
 * to float32 when out_bytes == 4: bit-equal to numpy's
 * `s.astype(float64) / float64(T) * scaler` (and its `.astype(float32)`).  A
 * sample with T == 0 (no rows, all zeros, cap == 0) is a row of +0.0, never NaN.
 * Every element of d_out is written once; nothing outside it is.
 * The table is checked on the device before anything is written: if for some s
 * d_lo[s] + d_n[s] wraps or exceeds n_rows, then *d_status = 2 and no byte of
 * d_out is written; otherwise *d_status = 0.  KF_EINVAL, before any HIP call,
 * for count_bytes not 2 or 4, out_bytes not 4 or 8, nbins == 0, n_samples < 0, a
 * scaler that is not finite, a null pointer (d_counts may be null when n_rows ==
 * 0) or a misaligned one (count_bytes for d_counts, 8 bytes for d_lo, d_n and
 * d_work, out_bytes for d_out, 4 for d_status).  KF_ERANGE if work_bytes <
 * kf_chunk_features_scratch_bytes(n_samples); the message says what is needed.
 * n_samples == 0 writes *d_status = 0 and nothing else.
 * Threads run along the columns with 16-byte loads where nbins is a multiple of
 * 16 / count_bytes and d_counts and d_out are 16-byte aligned (any other call
 * takes a scalar path with the same result).  nbins <= 8192 (every k <= 7): one
 * launch, a workgroup per sample sums its rows, reduces T and divides, the rows
 * read once.  Larger nbins: one memset of the totals and two launches, the first
 * adds (sample, column tile) sums to the sample's total with integer atomics
 * (order-independent, so the result is deterministic), the second sums the rows
 * again and divides.  Asynchronous on `stream`, no allocation, no host
 * synchronisation, no workgroup waits for another; at most one memset and two
 * kernel launches. */
uint64_t kf_chunk_features_scratch_bytes(int32_t n_samples);
int kf_chunk_features(const void* d_counts, int count_bytes, uint64_t n_rows, uint64_t nbins,
                      const uint64_t* d_lo, const uint64_t* d_n, int32_t n_samples,
                      uint32_t cap, double scaler, void* d_out, int out_bytes,
                      uint32_t* d_status, void* d_work, uint64_t work_bytes, void* stream);

/* ---- the same samples from a store of one byte per count (the reference's -cap:
 * utils.my_read_csv_chunk_capped keeps min(count, 255) as uint8 to halve the memory
 * of the whole library's window rows):
 *   d_counts         : n_rows x nbins u8 counts, row-major, already capped
 * and every other argument as kf_chunk_features', without count_bytes and cap.
 * For every table, scaler and out_bytes, d_out equals kf_chunk_features' on the
 * same values widened to u16 with cap = UINT32_MAX, bit for bit; so it also equals
 * kf_chunk_features with cap = 255 on the uncapped u16 rows these were made from
 * (kf_rows_cap8).  The sums are exact for any d_n; T == 0, the table check
 * (*d_status = 2, no byte written), n_samples == 0, KF_EINVAL and KF_ERANGE (the
 * messages start with "kf_chunk_features8: "; d_counts needs no alignment) and the
 * scratch (kf_chunk_features_scratch_bytes) are kf_chunk_features'.
 * The same kernels over 16 columns per 16-byte load, where nbins is a multiple of
 * 16 and d_counts and d_out are 16-byte aligned: two loads per row and thread,
 * eight rows in flight; the bytes are added two to a 32-bit word and these 16-bit
 * partial sums folded into the 64-bit sums every 256 rows, before one can wrap.
 * Any other call takes the scalar path with the same result.  At most one memset
 * and two launches, as kf_chunk_features. */
int kf_chunk_features8(const uint8_t* d_counts, uint64_t n_rows, uint64_t nbins,
                       const uint64_t* d_lo, const uint64_t* d_n, int32_t n_samples,
                       double scaler, void* d_out, int out_bytes,
                       uint32_t* d_status, void* d_work, uint64_t work_bytes, void* stream);

/* d_dst[i] = min(d_src[i], 255) for i < n: u16 window rows to the u8 rows of
 * kf_chunk_features8.  One streaming launch, 16-byte loads and stores where the
 * pointers allow (d_dst may have any alignment: the elements up to its next
 * 16-byte line and those behind the last whole group go one by one).  n == 0 is
 * a no-op.  KF_EINVAL for a null pointer or an odd d_src.  The arrays must not
 * overlap.  Asynchronous on `stream`, no allocation, no host synchronisation. */
int kf_rows_cap8(const uint16_t* d_src, uint64_t n, uint8_t* d_dst, void* stream);

/* ---- get_chunks `.kf` text parsed on the device into the uint16 window rows the
 * chunk trainers hold after my_read_csv_chunk (kf2vec/utils.py:402-405: pandas
 * read_csv with dtype=uint16), for many files or pieces of files per call:
 *   d_bytes, d_goff  : n_units units of text back to back (counter.pack_ranges'
 *                      layout: 16-byte aligned, padded with '\n'); unit u is
 *                      d_bytes[d_goff[u], d_goff[u+1]), a file or a piece of one
 *                      cut at line starts.  Unit edges are taken from the offsets
 *                      alone: a unit start is a line start and a unit end a line
 *                      end whether a '\n' is there or not (a unit whose size is a
 *                      multiple of 16 has no padding).
 *   d_rows           : cap_rows x nbins, row-major
 *   d_unit_row0      : n_units + 1 words: unit u's rows are [row0[u], row0[u+1])
 *   d_status         : 4 words: code, unit, row within the unit, column
 *   d_scratch        : kf_parse_kf_scratch_bytes(batch_bytes, n_units, cap_rows)
 * Lines and rows: a line starts at a unit start or after a '\n' and ends before
 * the next '\n' or at the unit end.  An empty line is no row (the padding makes
 * such lines); every other line is a row, numbered in byte order.
 * Fields: a row is a name followed by exactly nbins fields.  The name is every
 * byte up to the row's first ',' (any bytes but ',' and '\n'; it may be empty and
 * is not looked at); each field is preceded by ','.
 * Field form: one or more decimal digits, then optionally '.' and zero or more
 * '0'; the value is at most 65535 (accumulated so that a long digit string cannot
 * wrap; leading zeros are fine).  That is what kf_write_kf_segments{,16} write
 * without pseudocount ("16.0", or "16" for a row with no empty bin) and what
 * my_read_csv_chunk reads without error.  It is NARROWER than pandas: exponents,
 * signs, blanks, '\r' and fractions other than zeros are refused here, where
 * pandas would accept some of them for other dtypes; get_chunks writes none.
 * Results: d_rows[r * nbins + j] = field j of row r; d_unit_row0 as above; on
 * success d_status[0..3] = 0.
 * Errors: d_status[0] is the code of the error at the lowest byte offset,
 *   1 too few fields   (column = the number of fields the row has; at the row end)
 *   2 too many fields  (column = nbins; at the ',' that starts field nbins)
 *   3 malformed field  (column = the field; at its first offending byte, an empty
 *                       field's being the byte that ends it)
 *   4 value above 65535 (column = the field; at the digit that passes it)
 *   5 more rows than cap_rows (the row numbered cap_rows, column 0; rows from
 *                       that one on are not parsed)
 * with d_status[1] the unit, d_status[2] the row counted within the unit and
 * d_status[3] the column.  After an error the contents of d_rows are
 * unspecified (within its bounds); after code 5 the entries of d_unit_row0 are
 * capped at cap_rows + 1.
 * Memory safety: for any input bytes whatever, nothing outside d_rows[0, cap_rows
 * * nbins), d_unit_row0[0, n_units], d_status[0, 4) and d_scratch is written and
 * nothing outside d_bytes[0, batch_bytes) and d_goff[0, n_units] is read (unit
 * ends are clamped to batch_bytes).
 * KF_EINVAL, before any HIP call, for nbins == 0, n_units < 0, batch_bytes >=
 * 2^32, a null pointer or a misaligned one (16 bytes for d_bytes, 2 for d_rows, 8
 * for d_goff, d_unit_row0, d_status and d_scratch); KF_ERANGE if scratch_bytes is
 * below kf_parse_kf_scratch_bytes (the message says what is needed), which is 16
 * bytes + a word per 4 KiB of text + a word per row up to min(cap_rows,
 * batch_bytes) and does not decrease when an argument grows.
 * Five launches: the line starts of non-empty lines are compacted into a table
 * (count per 4 KiB, scan, scatter), then workgroups take rows grid-stride, each
 * walking its row in 4 KiB tiles of aligned 16-byte loads (a thread parses the
 * fields that start in its 16 bytes), and one workgroup writes d_unit_row0 and
 * the status.  A row is one workgroup's work, so few long rows (k >= 9) fill the
 * device less than many short ones.  Asynchronous on `stream`, no allocation, no
 * memset, no host synchronisation, no workgroup waits for another.
 * Measured on one MI355X, 1 GiB of text resident (tools/kf_parse_bench.py,
 * profiles/r14/): k=7 3.2 ms (335 GB/s of text; the text read three times plus
 * the rows written = 0.21 of the kf_stream_probe rate), k=3 25.6 ms (0.03: a
 * workgroup per 240-byte row); DESIGN.md section 4 has the table. */
uint64_t kf_parse_kf_scratch_bytes(uint64_t batch_bytes, int32_t n_units, uint64_t cap_rows);
int kf_parse_kf_rows(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_units,
                     uint64_t batch_bytes, uint64_t nbins, uint64_t cap_rows,
                     uint16_t* d_rows, uint64_t* d_unit_row0, uint64_t* d_status,
                     void* d_scratch, uint64_t scratch_bytes, void* stream);

/* ---- get_frequencies `.kf` text parsed on the device into the float64 feature
 * rows the trainers hold after my_read_csv (kf2vec/utils.py:436-437: pandas
 * read_csv, index_col=0, header=None) and `* features_scaler`, for many files or
 * pieces of files per call.  It follows kf_parse_kf_rows in everything but the
 * field and the output: d_bytes, d_goff, units, lines and rows, the name, exactly
 * nbins fields per row, d_unit_row0, d_status and its codes 1, 2, 3 and 5, "the
 * error at the lowest byte offset wins", and the memory safety are as stated
 * there.  What differs:
 *   d_vals     : cap_rows x nbins values of val_bytes bytes, row-major: 8 float64,
 *                4 float32
 *   d_row_name : 2 x cap_rows uint32: d_row_name[2r] is the byte offset of row r's
 *                name in the batch, d_row_name[2r + 1] its length (the bytes up to
 *                the row's first ','); the caller takes the names from its own
 *                copy of the text
 *   d_scratch  : kf_parse_kf_floats_scratch_bytes(batch_bytes, n_units, cap_rows)
 * Field form: digits [ '.' digits* ] [ ('e' | 'E') [ '+' | '-' ] digits ], with
 * `digits` one or more decimal digits -- what repr(float64) and "%d" write -- or
 * the three bytes "nan".  Signs on the significand, blanks, '\r', "inf",
 * "NaN", hex and a significand that starts with '.' are refused (code 3 at the
 * first offending byte): no writer of `.kf` files emits them.
 * Value: the digits before and after the '.' are one decimal significand w;
 * leading zeros (before or after the '.') are not significant.  From the first
 * digit that is not '0' on, every digit counts -- a trailing run of zeros too,
 * it is not folded into the exponent -- and there may be at most 19 of them, so
 * w is exact in 64 bits (repr writes at most 17).  q is the explicit exponent
 * minus the number of digits after the '.'; the exponent's magnitude saturates
 * at 99999 and the count of fraction digits at 2^20, so no digit string wraps
 * (either saturation leaves q outside the range below).  The field's value is
 * the binary64 nearest to w * 10^q, ties to even -- Python's float(field), bit
 * for bit -- by the Eisel-Lemire conversion of csrc/kf_decimal.h, which covers
 * -342 <= q <= 308 and every uint64 w.  w == 0 gives 0.0 whatever q is; "nan"
 * gives the quiet NaN 0x7FF8000000000000.
 * Results: d_vals[r * nbins + j] = value * scaler, one float64 multiply (the
 * trainers' `* features_scaler`), stored as float64 or rounded once more to
 * float32 (to nearest even; above FLT_MAX it is infinite, as numpy's astype);
 * d_row_name and d_unit_row0 as above; on success d_status[0..3] = 0.
 * Errors: the codes of kf_parse_kf_rows but 4, which is not used, and
 *   6 more than 19 significant digits (column = the field; at the digit that
 *                       passes the limit)
 *   7 magnitude outside the normal float64 range (column = the field; at the
 *                       byte that ends it, before a code 2 at that byte): w != 0
 *                       and w * 10^q below 2^-1022 -- subnormals are not
 *                       produced, and a decimal just below 2^-1022 is not
 *                       rounded up to it -- or rounding to more than DBL_MAX, or
 *                       q outside [-342, 308]
 * After an error the contents of d_vals and d_row_name are unspecified (within
 * their bounds); a row without a ',' (code 1, column 0) has no name entry.
 * Memory safety as kf_parse_kf_rows: nothing outside d_vals[0, cap_rows * nbins),
 * d_row_name[0, 2 * cap_rows), d_unit_row0[0, n_units], d_status[0, 4) and
 * d_scratch is written, for any input bytes whatever.
 * KF_EINVAL, before any HIP call, for nbins == 0, n_units < 0, val_bytes other
 * than 4 and 8, batch_bytes >= 2^32, a null pointer or a misaligned one (16
 * bytes for d_bytes, val_bytes for d_vals, 4 for d_row_name, 8 for d_goff,
 * d_unit_row0, d_status and d_scratch); KF_ERANGE if scratch_bytes is below
 * kf_parse_kf_floats_scratch_bytes, which is kf_parse_kf_scratch_bytes plus the
 * 10,416 bytes of the table of powers of five and does not decrease when an
 * argument grows.
 * One small copy and five launches: the table of powers of five (computed on the
 * host on first use, once per process) is copied to the head of the scratch on
 * `stream`, so a call leaves no state on the device; then kf_parse_kf_rows'
 * passes with this field parser.  A row is one workgroup's work and a thread
 * parses the fields that start in its 16 bytes: a float field is longer than
 * that, so most threads parse one field or none, and a directory of thousands
 * of genome rows fills the device where one row would not.  The launches are
 * asynchronous on `stream`: no allocation, no memset, no wait for the device, no
 * workgroup waits for another.  The copy of the table is a hipMemcpyAsync whose
 * source is pageable host memory (the table never changes once built): the
 * runtime stages its 10 KiB, so the host may wait for that staging copy, though
 * not for the work queued on the device, and a stream that is being captured
 * into a graph cannot take this call.
 * Measured on one MI355X, 1 GiB of text resident (tools/kf_float_bench.py,
 * profiles/r18/kf_float_k7.json): k=7, 5,839 rows, 7.1 ms (151 GB/s of text; 2.2
 * times kf_parse_kf_rows' time per byte of text in the same run), k=3 30.0 ms
 * (1.3 times), k=9 16.9 ms (4.1 times: 366 rows for 2,048 workgroup slots);
 * DESIGN.md section 4 has the table. */
uint64_t kf_parse_kf_floats_scratch_bytes(uint64_t batch_bytes, int32_t n_units, uint64_t cap_rows);
int kf_parse_kf_floats(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_units,
                       uint64_t batch_bytes, uint64_t nbins, uint64_t cap_rows, double scaler,
                       void* d_vals, int val_bytes, uint32_t* d_row_name,
                       uint64_t* d_unit_row0, uint64_t* d_status,
                       void* d_scratch, uint64_t scratch_bytes, void* stream);

/* The conversion that kf_parse_kf_floats runs per field, on the host (the same
 * inline code, csrc/kf_decimal.h): out[i] = the binary64 nearest to w[i] *
 * 10^q[i], ties to even, and in_range[i] = 1; or in_range[i] = 0 and out[i] =
 * 0.0 where the contract above reports code 7.  KF_EINVAL for a null pointer
 * with n > 0. */
int kf_decimal_to_double(const uint64_t* w, const int32_t* q, uint64_t n, double* out, uint8_t* in_range);

/* ---- tab-separated tables of decimal floats parsed on the device: the true
 * distance matrix of a clade (`<tree>_subtree_<c>.di_mtrx`, read by both distance
 * trainers with pandas read_csv(sep='\t', header=0, index_col=0) and reindexed by
 * kf2vec/utils.py:141-192) and the backbone embeddings
 * (`embeddings_subtree_<c>.csv`, kf2vec/query.py:129-134), for many pieces of a
 * file per call.  The header line of a `.di_mtrx` is the caller's: the units hold
 * the rows alone.  It follows kf_parse_kf_floats in everything not listed here:
 * d_bytes, d_goff, units and their edges, lines and rows, empty lines,
 * d_row_name, d_unit_row0, d_status and "the error at the lowest byte offset
 * wins", the 19 significant digits, the value of a decimal, the memory safety for
 * any input bytes, the scratch layout, the copy of the powers of five and the
 * five launches, asynchronous on `stream` without allocation or host wait (and,
 * for the copy's pageable source, not under graph capture).  What differs:
 * Separator: '\t'.  The name is every byte up to the row's first '\t' (any bytes
 * but '\t' and '\n': it may hold ',' and blanks and may be empty); each of the
 * row's exactly `ncols` fields is preceded by '\t' (codes 1 and 2 as there, the
 * column of code 2 being ncols).
 * Field form: [ '-' ] digits [ '.' digits* ] [ ('e' | 'E') [ '+' | '-' ] digits ],
 * or the three bytes "nan".  A '-' is taken only as a field's first byte; "-nan"
 * (at its 'n'), a lone "-" (at the byte that ends it), "+1", "1-", "inf", blanks,
 * ',' and '\r' are code 3 at the first offending byte.
 * Value: the binary64 nearest to the decimal, ties to even, its sign bit set if
 * the field began with '-': "-0.0" gives 0x8000000000000000.  There is no scaler.
 * val_bytes == 4 rounds that value once more to float32, as numpy's astype.
 * Columns: field j of row r goes to d_vals[r * out_cols + d_col_map[j]].
 *   d_col_map : ncols int32 on the device.  An entry outside [0, out_cols) means
 *               "skip this column": the field is still checked for form and digit
 *               count (codes 3 and 6) but is not converted, so code 7 is never
 *               reported for it.  NULL is the identity, and out_cols must then
 *               equal ncols.
 *   d_vals    : cap_rows x out_cols values of val_bytes bytes, row-major.  Entries
 *               that no field maps to are not written (the caller pre-fills them);
 *               two columns mapped to one destination leave it holding either
 *               value.  Nothing outside d_vals[0, cap_rows * out_cols) is written,
 *               whatever the map holds.
 * Errors: codes 1, 2, 3, 5, 6 and 7 of kf_parse_kf_floats with the same columns
 * (the file's column j, not its destination); no other code.
 * KF_EINVAL, before any HIP call, for ncols == 0, out_cols == 0, d_col_map ==
 * NULL with out_cols != ncols, n_units < 0, val_bytes other than 4 and 8,
 * batch_bytes >= 2^32, a null pointer (but d_col_map) or a misaligned one (16
 * bytes for d_bytes, val_bytes for d_vals, 4 for d_col_map and d_row_name, 8 for
 * d_goff, d_unit_row0, d_status and d_scratch); KF_ERANGE if scratch_bytes is
 * below kf_parse_tsv_floats_scratch_bytes, which equals
 * kf_parse_kf_floats_scratch_bytes and does not decrease when an argument grows.
 * A row is one workgroup's work, as there: an N x N matrix is N rows of about 19
 * N bytes.  Measured on one MI355X (tools/tsv_bench.py,
 * profiles/r19/tsv_floats.json): a 4,000 x 4,000 matrix, 301 MB of text resident,
 * about 1.7 ms (170 GB/s of text), 1.8 ms with a shuffled map; three quarters of
 * kf_parse_kf_floats' time per byte on k=7 text of the same size in the same run
 * (whose 1,639 rows leave a fifth of the workgroup slots empty); DESIGN.md
 * section 4 has the table. */
uint64_t kf_parse_tsv_floats_scratch_bytes(uint64_t batch_bytes, int32_t n_units, uint64_t cap_rows);
int kf_parse_tsv_floats(const uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_units, uint64_t batch_bytes,
                        uint64_t ncols, const int32_t* d_col_map, uint64_t out_cols, uint64_t cap_rows,
                        void* d_vals, int val_bytes, uint32_t* d_row_name,
                        uint64_t* d_unit_row0, uint64_t* d_status,
                        void* d_scratch, uint64_t scratch_bytes, void* stream);

/* ---- get_chunks `.kf` text formatted on the device: the inverse of
 * kf_parse_kf_rows, and the lines of kf_write_kf_segments16 for raw counts
 * (raw_cnt = 1; format_line in kf_host.cpp, main.py:344-357 and :905-915).
 * Row r of d_counts[n_rows x nbins] (uint16) becomes one line; the lines stand
 * back to back in d_text:
 *   name ',' col_0 ',' ... ',' col_{nbins-1} '\n'
 * name: prefix p = d_row_prefix[r], the bytes d_prefix_bytes[d_prefix_off[p],
 * d_prefix_off[p + 1]) (any bytes, maybe none), followed, if win_len != 0, by
 * dec(s + 1) '-' dec(s + win_len) for s = d_row_start[r] (uint64 arithmetic,
 * wrapping); win_len == 0: the prefix alone, so a caller can pass whole names.
 * column text of a count c: "c.5" with pseudocount, else "c.0"; without
 * pseudocount a row with no zero column, or with only zero columns, is written
 * as integer text "c" in every column (at k=3 nearly every 10 kbp window is).
 * A line is at most name_len + 1 + 8 * nbins bytes ("65535.0,"), and a name at
 * most its prefix + 41 bytes: callers size cap_bytes by that.
 * d_row_off[r] = the byte offset of row r's line, d_row_off[n_rows] the total.
 * d_status[0, 4) = code, bytes needed, row, 0:
 *   0 ok (d_status[1] = the total)
 *   1 the text is longer than cap_bytes: d_status[1] is the size needed,
 *     d_row_off is still complete, the contents of d_text are unspecified
 *     (within its bounds)
 *   2 d_row_prefix[r] >= n_prefixes, or d_prefix_off is not non-decreasing:
 *     d_status[2] is the first row whose prefix is out of range or has
 *     d_prefix_off[p] > d_prefix_off[p + 1] (n_rows if the decreasing entries are
 *     no row's prefix); nothing is formatted, d_row_off[n_rows] = 0 and the
 *     other entries of d_row_off are unspecified.
 * Memory safety, for any input whatever: nothing is written outside d_text[0,
 * cap_bytes), d_row_off[0, n_rows], d_status[0, 4) and d_scratch; nothing is read
 * outside d_counts[0, n_rows * nbins), d_prefix_off[0, n_prefixes], the prefix
 * bytes of a call that is not refused, and d_row_prefix, d_row_start[0, n_rows).
 * KF_EINVAL, before any HIP call, for nbins == 0, n_rows >= 2^31, cap_bytes >=
 * 2^32 (offsets inside a call fit 32 bits: the caller cuts a launch's rows into
 * calls), n_prefixes < 0, n_rows * nbins >= 2^42, a null pointer with n_rows > 0
 * (d_row_off and d_status always), or a misaligned pointer (2 bytes for d_counts,
 * 4 for d_row_prefix, 8 for d_prefix_off, d_row_start, d_row_off, d_status and
 * d_scratch; d_text and d_prefix_bytes need none); KF_ERANGE if scratch_bytes is
 * below kf_format_kf_scratch_bytes (the message says what is needed), which is
 * 16 bytes + 16 per row + 8 per 2,048 cells and does not decrease when an
 * argument grows.  n_rows == 0 is valid: d_row_off[0] = 0, status 0.
 * Six launches (five with pseudocount): the prefix table is checked, a thread
 * per row checks its prefix and stores its name's length, then the flat cell
 * array is walked three times in tiles of 2,048 cells (8 per thread, whatever
 * nbins is): the zero columns of every row (which decide its form), the text
 * length of every tile, and -- after one workgroup scanned those -- the text,
 * staged in LDS and stored as aligned 16-byte lines with byte stores at a
 * tile's ragged ends.  Asynchronous on `stream`, no allocation, no memset, no
 * host synchronisation, no workgroup waits for another.
 * Measured on one MI355X, one count launch's rows (tools/kf_format_bench.py,
 * profiles/r17/): k=7, 4,096 x 8,192 cells, 134 MB of text in 0.27 ms (500
 * GB/s of text, 5.6 times a device copy of the text); k=3 0.037 ms; k=10, 511 x
 * 524,800 cells, 1.07 GB in 1.64 ms; DESIGN.md section 4 has the table. */
uint64_t kf_format_kf_scratch_bytes(uint64_t n_rows, uint64_t nbins);
int kf_format_kf_rows16(const uint16_t* d_counts, uint64_t n_rows, uint64_t nbins,
                        const uint8_t* d_prefix_bytes, const uint64_t* d_prefix_off, int32_t n_prefixes,
                        const uint32_t* d_row_prefix, const uint64_t* d_row_start, uint32_t win_len,
                        int pseudocount,
                        uint8_t* d_text, uint64_t cap_bytes, uint64_t* d_row_off, uint64_t* d_status,
                        void* d_scratch, uint64_t scratch_bytes, void* stream);

/* ---- tables of floats formatted on the device: the inverse of
 * kf_parse_kf_floats and kf_parse_tsv_floats, and the text of query's two
 * tables (kf2vec/query.py:178-192: .tolist() and csv.writer), of the trainers'
 * to_csv tables of float32 frames (train_model_set.py:630-643) and of `.di_mtrx`
 * files.  Row r of d_vals[n_rows x ncols] (float32 or float64 by val_bytes, row
 * major) becomes one line; the lines stand back to back in d_text:
 *   prefix_r sep f_0 sep ... sep f_{ncols-1} eol
 * prefix_r: the bytes d_prefix_bytes[d_prefix_off[p], d_prefix_off[p + 1]) for p
 * = d_row_prefix[r] (any bytes: the host quotes labels before it passes them);
 * an empty prefix writes no leading separator.  sep: one byte, not NUL.  eol:
 * eol_len = 1 or 2 bytes, the first in the low byte of `eol` ("\r\n" = 0x0A0D:
 * csv.writer; "\n" = 0x0A: pandas).
 * f: the shortest decimal that reads back as the value (csrc/kf_shortest.h:
 * Schubfach), of the shortest candidates the closest, at most 24 bytes:
 *   mode KF_FLOAT_SHORTEST, val_bytes 8   Python's repr(float)
 *   mode KF_FLOAT_SHORTEST, val_bytes 4   numpy's str(np.float32) (at most 9
 *                                         digits), which is also pandas' to_csv
 *   mode KF_FLOAT_WIDENED,  val_bytes 4   repr of the float32 converted to
 *                                         double: .tolist() then csv.writer
 * Fixed notation for 1e-4 <= |v| < 1e16 (repr decides by the decimal's exponent,
 * numpy by the value: float32(1e-4) is "1e-04"), integral values with ".0", else
 * d[.ddd]e+XX / e-XX with at least two exponent digits; "0.0", "-0.0", "inf",
 * "-inf"; a NaN of either sign is "nan", or with nan_empty != 0 an empty field
 * (pandas' na_rep).  Every float32 and every float64 is formatted, subnormals
 * included.
 * d_row_off[r] = the byte offset of row r's line, d_row_off[n_rows] the total.
 * d_status[0, 4) = code, bytes needed, row, column:
 *   0 ok (d_status[1] = the total)
 *   1 the text is longer than cap_bytes: d_status[1] is the size needed,
 *     d_row_off is still complete, the contents of d_text are unspecified
 *     (within its bounds)
 *   2 d_row_prefix[r] >= n_prefixes, or d_prefix_off is not non-decreasing:
 *     d_status[2] as for kf_format_kf_rows16; nothing is formatted,
 *     d_row_off[n_rows] = 0
 *   3 reserved for a value that cannot be formatted; no value is refused
 * A line is at most prefix + 1 + 25 * ncols + 1 bytes: callers size cap_bytes by
 * that, or call twice.  Memory safety, for any input whatever: nothing is
 * written outside d_text[0, cap_bytes), d_row_off[0, n_rows], d_status[0, 4) and
 * d_scratch; nothing is read outside d_vals[0, n_rows * ncols), d_prefix_off[0,
 * n_prefixes], the prefix bytes of a call that is not refused, and
 * d_row_prefix[0, n_rows).
 * KF_EINVAL, before any HIP call, for val_bytes other than 4 and 8, a mode that
 * val_bytes does not have, ncols == 0, sep outside 1..255, eol_len other than 1
 * and 2, n_rows >= 2^31, cap_bytes >= 2^32 (the caller cuts rows into calls),
 * n_prefixes < 0, n_rows * ncols >= 2^34 (a launch has fewer than 2^32 threads), a null pointer with n_rows > 0
 * (d_row_off and d_status always), or a misaligned pointer (val_bytes for d_vals,
 * 4 for d_row_prefix, 8 for d_prefix_off, d_row_off, d_status and d_scratch;
 * d_text and d_prefix_bytes need none); KF_ERANGE if scratch_bytes is below
 * kf_format_float_scratch_bytes, which is the table of powers of ten (9,872
 * bytes) + 16 + 8 per row + 8 per kf_format_float_tile() = 1,024 cells + 16
 * per cell (every cell's decimal, kept between the two walks) and does not
 * decrease when an argument grows.  n_rows == 0 is valid: d_row_off[0] = 0,
 * status 0.
 * Five launches and the copy of the table: the prefix table is checked, a
 * thread per row stores its prefix's length, then the flat cell array is walked
 * twice in tiles of 1,024 cells (4 per thread, whatever ncols is): the text
 * length of every tile, and -- after one workgroup scanned those -- the text,
 * staged in LDS and stored as aligned 16-byte lines with byte stores at a
 * tile's ragged ends.  The first walk computes a cell's digits and keeps them
 * in the scratch, the second reads them back (measured against computing them
 * twice: DESIGN.md section 7).  Asynchronous on `stream`, no allocation, no memset, no
 * host synchronisation, no workgroup waits for another.
 * kf_format_float_host: the same inline code on the host for n values: slot i
 * of out (24 bytes, zero padded) and len[i]; kf_shortest_decimal_host: the
 * decimal behind the text, w[i] * 10^q[i] (w == 0 unless finite and non-zero)
 * and cls[i] = class (0 finite, 1 zero, 2 inf, 3 nan) | sign << 7.  The CPU tests
 * call them, as they call kf_decimal_to_double for the parser. */
#define KF_FLOAT_SHORTEST 0
#define KF_FLOAT_WIDENED 1
int kf_format_float_tile(void);
uint64_t kf_format_float_scratch_bytes(uint64_t n_rows, uint64_t ncols);
int kf_format_float_rows(const void* d_vals, int val_bytes, uint64_t n_rows, uint64_t ncols, int mode,
                         uint32_t sep, uint32_t eol, int eol_len, int nan_empty,
                         const uint8_t* d_prefix_bytes, const uint64_t* d_prefix_off, int32_t n_prefixes,
                         const uint32_t* d_row_prefix,
                         uint8_t* d_text, uint64_t cap_bytes, uint64_t* d_row_off, uint64_t* d_status,
                         void* d_scratch, uint64_t scratch_bytes, void* stream);
int kf_format_float_host(const void* vals, int val_bytes, int mode, int nan_empty, uint64_t n,
                         uint8_t* out, uint8_t* len);
int kf_shortest_decimal_host(const void* vals, int val_bytes, int mode, uint64_t n,
                             uint64_t* w, int32_t* q, uint8_t* cls);

/* ---- query's distances (kf2vec/query.py:169-176): out[i, j] for x[Q x D] and
 * y[B x D], float32, contiguous, is exactly
 *   s = 0; for d ascending: t = x_d - y_d, s = s + t * t; r = sqrt(s); v = r * r;
 *   out = v < 1e-6f ? 0 : v
 * with every operation rounded to float32 and none contracted into an fma: the
 * direct form of torch.cdist(compute_mode='donot_use_mm_for_euclid_dist'),
 * squared and cut as the reference does, which keeps the digits of small
 * distances that the matmul form cancels.  The order over d is fixed, so the
 * result does not depend on how Q and B are cut into tiles or into calls.
 * Tiles of kf_sq_distances_tile() = 64 rows of x and of y go through LDS, read
 * from HBM once per tile pair.  No scratch; asynchronous on `stream`.
 * KF_EINVAL, before any HIP call, for D == 0, a null pointer that the sizes
 * need, a pointer not aligned to 4 bytes, or 2^24 tiles or more (a launch has
 * fewer than 2^32 threads: the caller cuts Q or B).  Q == 0 or B ==
 * 0 is valid and writes nothing. */
int kf_sq_distances_tile(void);
int kf_sq_distances(const float* d_x, uint64_t Q, const float* d_y, uint64_t B, uint64_t D,
                    float* d_out, void* stream);

/* ---- classify's class probabilities (kf2vec/classify.py:117-122): for each row
 * of d_logits[Q x C], float32, contiguous, with every operation rounded to
 * float32 and none contracted into an fma,
 *   m = max_j x_j; t_j = x_j - m; e_j = expf(t_j); s = sum_j e_j; p_j = e_j / s
 * (a correctly rounded division): torch.exp(F.log_softmax(x, dim=1)) in the
 * direct form, which keeps the digits of small probabilities that
 * exp(x - m - log s) loses.  d_out[r, 1 + j] = p_j; d_top[r] = the lowest j
 * whose rounded p_j is the row's largest (topk(1)'s choice among ties on the
 * CPU); d_out[r, 0] = p[d_top[r]], the same bits: the C + 1 floats that a row
 * of classes.out holds behind its label and class, ready for
 * kf_format_float_rows.
 * A row that holds a NaN or +inf, or is all -inf, is NaN in all C + 1 outputs
 * with d_top = 0 (IEEE evaluation of the lines above; an empty genome's NaN
 * features end here); a -inf among finite logits has p = 0.
 * A wave owns a row, kf_class_probs_rows() = 4 rows per workgroup.  A lane adds
 * its columns (l, l + 64, ...) in ascending order and the 64 partial sums meet
 * in an xor butterfly, so the sum is a fixed function of C alone: a row's bits
 * depend neither on Q, nor on its place, nor on how Q is cut into calls.  Up to
 * kf_class_probs_reg_cols() = 1024 columns the row stays in registers, above
 * that it is read three times.  No scratch, no memset, no allocation, no host
 * synchronisation; asynchronous on `stream`.
 * KF_EINVAL, before any HIP call, for C == 0, C >= 2^31, Q above 4 * (2^24 - 1)
 * (a launch has fewer than 2^32 threads: the caller cuts Q), a null pointer
 * with Q > 0, or a pointer not aligned to 4 bytes.  Q == 0 is valid and writes
 * nothing. */
int kf_class_probs_reg_cols(void);
int kf_class_probs_rows(void);
int kf_class_probs(const float* d_logits, uint64_t Q, uint64_t C, float* d_out /* [Q x (C+1)] */,
                   int32_t* d_top /* [Q] */, void* stream);

/* ---- the distance trainer's loss and its gradient (kf2vec/train_model_set.py:448-467,
 * losses.py:13-49, utils.py:240-256): for the batch's embeddings d_y[B x E] (float32,
 * contiguous), the clade's true distances d_true[N x N] (float64, contiguous) and the
 * batch's labels d_labels[B] (rows and columns of d_true), over i, j in [0, B), with
 * every operation rounded on its own and none contracted into an fma,
 *   s_ij = 0; for e ascending: t = y_i[e] - y_j[e], s = s + t * t          (float32)
 *   d_ij = sqrtf(s_ij)                                                     (correctly rounded)
 *   T = d_true[l_i * N + l_j]; w = 1.0 / (T + 1e-6); r = sqrt(T); u = (double)d_ij - r
 *   v_ij = (u * u) * w; inv = 1.0 / (double)(B * B)                        (float64)
 *   *d_loss = (sum_i (sum_j v_ij)) * inv
 *       (float64; both sums start at 0.0, the inner over j ascending, the outer over i
 *       ascending; the diagonal is included, as .mean() includes it)
 *   g_ij = (float)(((2.0 * u) * w) * inv)
 *   c_ij = d_ij == 0 ? 0 : (g_ij + g_ji) / d_ij
 *       (float32, a correctly rounded division; g_ji is taken at d_true[l_j * N + l_i]:
 *       the matrix need not be symmetric; a zero distance gives a zero gradient, as
 *       cdist's backward does)
 *   d_grad[i, e] = 0; for j ascending: grad = grad + c_ij * (y_i[e] - y_j[e])   (float32)
 * This is torch.cdist(y, y, compute_mode='donot_use_mm_for_euclid_dist'), the
 * reference's Loss.my_mse_loss and autograd's backward of both down to y, in the direct
 * form.  Every output's chain of additions is walked by one thread in the stated order,
 * so the bits depend neither on tiles nor on the path taken, and two calls agree bit for
 * bit; train.dist_loss_host states the same operations in numpy.
 * NaN, negative or infinite entries of d_true and NaN embeddings follow IEEE
 * evaluation of the lines above; nothing is special-cased.  Repeated labels are valid.
 * A label outside [0, N) sets *d_status = 1 and makes *d_loss NaN (the gradient is then
 * NaN wherever a non-zero distance enters it, and not to be used: the caller goes by
 * the status), and nothing is read out of bounds; otherwise *d_status = 0.  d_grad == NULL
 * gives the loss alone, with the same bits (the test-set pass).
 * Up to kf_dist_loss_small_b() = 32 rows one workgroup does everything in one launch
 * and no scratch is needed (d_scratch may be NULL).  Above, five launches: d by tiles of
 * kf_dist_loss_tile() = 32 rows, E walked in slices of kf_dist_loss_depth() = 32
 * columns through LDS; one thread per pair; the row sums; the total with the labels'
 * check; and d_grad by tiles of 32 rows x 32 columns, j walked in slices of 32.
 * kf_dist_loss_scratch_bytes gives the scratch for B rows (12 * B * B + 8 * B bytes
 * above 32 rows).  The call allocates nothing, sets no memory and never waits for the
 * device: it is asynchronous on `stream`, and all scratch is the caller's.
 * KF_EINVAL, before any HIP call, for B == 0, E == 0, B above kf_dist_loss_max_b() =
 * 8192, E above 2^24, N == 0 or N >= 2^30, a null d_y, d_true, d_labels, d_loss or
 * d_status, a null d_scratch where scratch is needed, a scratch that is too small, or a
 * pointer not aligned to its element (8 bytes for d_true, d_labels, d_loss and
 * d_scratch, 4 for d_y, d_grad and d_status). */
int kf_dist_loss_small_b(void);
int kf_dist_loss_tile(void);
int kf_dist_loss_depth(void);
uint64_t kf_dist_loss_max_b(void);
int kf_dist_loss_scratch_bytes(uint64_t B, uint64_t* bytes);
int kf_dist_loss(const float* d_y, uint64_t B, uint64_t E,            /* embeddings [B x E] */
                 const double* d_true, uint64_t N,                    /* true distances [N x N] */
                 const int64_t* d_labels,                             /* [B], rows/cols of d_true */
                 double* d_loss, float* d_grad /* [B x E] or NULL */,
                 int32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* ---- the chunk trainer's loss and its gradient (kf2vec/train_model_set_chunks.py:392-418,
 * losses.py:58-117): kf_dist_loss' contract, line for line, with two changes.  `views`
 * rows that follow each other are views of one genome and share its label: row i's label
 * is d_labels[i / views] (torch.repeat_interleave(labels, views)), so d_labels holds
 * B / views entries.  And the weight is w = 1.0 / (T + eps), on the side of
 * T = d_true[l_i * N + l_j] and on that of d_true[l_j * N + l_i] (Loss_chunks has
 * eps = 1000).  The rest is kf_dist_loss': the float32 direct-form distances, the float64
 * pair terms, both sums in ascending order from 0.0, inv = 1.0 / (double)(B * B) over all
 * B rows with the diagonal and the pairs of one genome's views included, c_ij = 0 where
 * d_ij == 0 (two equal views), no fma, status 1 and a NaN loss for a label outside [0, N)
 * with nothing read out of bounds, d_grad == NULL for the loss alone, one workgroup up to
 * kf_dist_loss_small_b() rows (rows, not labels) and five launches above, the scratch of
 * kf_dist_loss_scratch_bytes(B), no allocation, memset or wait.  kf_dist_loss is this call
 * with views = 1 and eps = 1e-6, the same code and the same bits;
 * train.dist_loss_host(..., views, eps) states both in numpy.
 * KF_EINVAL, before any HIP call, for kf_dist_loss' cases and for views == 0, B no
 * multiple of views, and an eps that is NaN, infinite or negative. */
int kf_dist_loss_views(const float* d_y, uint64_t B, uint64_t E,      /* embeddings [B x E] */
                       const double* d_true, uint64_t N,              /* true distances [N x N] */
                       const int64_t* d_labels /* [B / views] */, uint64_t views, double eps,
                       double* d_loss, float* d_grad /* [B x E] or NULL */,
                       int32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* ---- the classifier trainer's loss, its gradient, the batch's right classes and the
 * epoch's totals (kf2vec/train_classifier_model.py:323-342): for the batch's logits
 * d_logits[B x C] (float32, contiguous; the output of fc3, the softmax is the kernel's)
 * and its classes d_true[B] (int64), per row i with c = d_true[i], every operation rounded
 * to float32 and none contracted into an fma,
 *   m = max_j x_j; t_j = x_j - m; e_j = expf(t_j); s = sum_j e_j; p_j = e_j / s
 *       (kf_class_probs' own lines, in its order of the sum -- lane l adds the columns l,
 *       l + 64, ... ascending, then the xor butterfly -- and with its correctly rounded
 *       division: p_j has the bits kf_class_probs writes)
 *   nll_i = logf(s) - t_c
 *   hit_i = (the lowest j whose p_j is the row's largest) == c       (kf_class_probs' d_top)
 *   g_ij  = (p_j - (j == c ? 1.0f : 0.0f)) * invB,  invB = 1.0f / (float)B
 * and per call
 *   *d_loss   = (sum_i (double)nll_i) * (1.0 / (double)B)
 *       (float64; the sum starts at 0.0 and one thread adds the rows with i ascending, on
 *       either path: the order is a fixed function of B alone)
 *   *d_hits   = sum_i hit_i
 *   *d_status = 1 if any d_true[i] is outside [0, C), else 0.
 * This is F.log_softmax, nn.NLLLoss() (mean), autograd's backward of both down to the
 * logits, and exp / topk(1) / accuracy_score, in the direct form;
 * train_classifier.class_loss_host states it in numpy.  d_grad[B x C] may be NULL: the loss
 * alone, the same bits.  d_row_loss[B] may be NULL; else it receives the nll_i.
 * d_totals[3] (float64) may be NULL; else the finishing thread does
 *   totals[0] += *d_loss * (double)B; totals[1] += *d_hits; totals[2] += *d_status
 * with plain loads and stores in stream order: calls that share a totals buffer must go on
 * one stream (no atomic is used, one thread does it), and the caller zeroes the buffer.
 * Against the float64 value of log(sum_j exp(t_j)) - t_c from the same float32 logits, with
 * T = sum_j p_j |t_j| (at most the largest finite |t_j|) and beside kf_class_probs'
 * (|t_j| + C + 8) * 2^-24:
 *   |nll_i - nll| <= (T + C + 8 + 4 |log s| + |t_c| + |nll|) * 2^-24 + C * 2^-126
 * -- s carries the subtractions' |t_j| * 2^-24 through exp, expf's 2 units and C - 1
 * additions of positives, relative, which log turns into an absolute error; logf is held to
 * 2 units of log s; t_c and the last subtraction are rounded once each; an e_j below
 * 2^-126 may be flushed to 0 while s >= 1.
 * A row that holds a NaN or +inf, or is all -inf (kf_class_probs' NaN rows), has nll_i NaN,
 * its gradient row NaN and hit_i 0; the loss is then NaN and the status 0.  A -inf logit
 * among finite ones has p = 0; if it is the true class, nll_i = +inf.  A class outside
 * [0, C) gives status 1, that row's nll_i and gradient row NaN and hit_i 0, and nothing is
 * read out of bounds.  C == 1 is valid (p = 1, nll = 0, g = 0).  Repeated classes are the
 * normal case.  A row's nll_i and p_j depend neither on B, nor on its place, nor on the path.
 * A wave owns a row, in kf_class_probs' register tiers (1, 4 or 16 values per lane, three
 * reads above kf_class_probs_reg_cols() columns).  Up to kf_class_loss_small_b() = 64 rows
 * one workgroup does everything in one launch and no scratch is needed (d_scratch may be
 * NULL).  Above, two launches: the rows (4 per workgroup) leave nll_i and hit_i in the
 * caller's scratch, and one workgroup finishes.  kf_class_loss_scratch_bytes gives the
 * scratch for B rows (8 * B bytes above 64 rows).  The call allocates nothing, sets no
 * memory and never waits for the device: it is asynchronous on `stream`.
 * KF_EINVAL, before any HIP call, for B == 0, C == 0, C >= 2^31, B above
 * kf_class_loss_max_b() = 65536, a null d_logits, d_true, d_loss, d_hits or d_status, a
 * null d_scratch where scratch is needed, a scratch that is too small, or a pointer not
 * aligned to its element (8 bytes for d_true, d_loss, d_totals and d_scratch, 4 for
 * d_logits, d_grad, d_row_loss, d_hits and d_status). */
int kf_class_loss_small_b(void);
uint64_t kf_class_loss_max_b(void);
int kf_class_loss_scratch_bytes(uint64_t B, uint64_t* bytes);
int kf_class_loss(const float* d_logits, uint64_t B, uint64_t C,      /* logits [B x C] */
                  const int64_t* d_true,                              /* [B], classes */
                  double* d_loss, float* d_grad /* [B x C] or NULL */, float* d_row_loss /* [B] or NULL */,
                  int32_t* d_hits, int32_t* d_status, double* d_totals /* [3] or NULL */,
                  void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Hash of the sources this library was built from (csrc/ + this header, as
 * kf2vecfsw_amd/build.py computes it): 16 hex digits, with a "+<tag>" suffix for
 * profiling builds.  The Python binding refuses a library whose id differs from
 * the sources next to it. */
const char* kf_build_id(void);

/* Measurement aid (bench.py): read d_bytes[0, n) with the fastest read pattern
 * measured on gfx950 (3 KiB blocks dealt grid-stride over the waves, coalesced
 * 16-byte lanes, four blocks in flight per wave) and XOR-fold it into *d_out
 * (device).  Time it to get the practical HBM read ceiling.  Needs n rounded up
 * to 16 readable. */
int kf_stream_probe(const uint8_t* d_bytes, uint64_t n, uint32_t* d_out, void* stream);

/* Free the large-k workspace and tables of the current device (synchronises the
 * device).  The next large-k kf_count_batch allocates them again. */
int kf_workspace_release(void);

/* Synthetic FASTA generator on the device (benchmark/test input; spec in
 * DESIGN.md "Synthetic genomes"): genome i has id g = g0 + i*g_stride (so a rank
 * of a round-robin shard passes g0 = rank, g_stride = world) and seed seed0 + g;
 * it is written to d_bytes[d_goff[i], d_goff[i+1]) as ">syn_<g>\n" + seq_len
 * bases in `width`-column lines + '\n' padding.  d_goff must be 16-aligned. */
int kf_synth_fasta(uint8_t* d_bytes, const uint64_t* d_goff, int32_t n_genomes,
                   int64_t g0, int64_t g_stride, uint64_t seed0, uint64_t seq_len,
                   int width, uint64_t n_period, void* stream);

/* Host-side layout for kf_synth_fasta: genome sizes rounded up to `align`. */
uint64_t kf_synth_genome_bytes(int64_t g, uint64_t seq_len, int width, uint64_t align);
uint64_t kf_synth_header_len(int64_t g);

/* One `.kf` line, byte-identical to main.py:331-357:
 *   "<name>," + ",".join(str(v)) + "\n"
 * with v = counts (+0.5 if pseudocount) (/ sum unless raw_cnt), float64,
 * printed like Python repr(float); raw counts with no empty bin print as
 * integers (pandas keeps int64 when the left-merge introduces no NaN), and so
 * do the zeros of a genome with no k-mer at all (an empty dump).
 * On KF_ERANGE *written is the size needed. */
int kf_format_kf(const char* name, const uint32_t* counts, uint64_t nbins,
                 int pseudocount, int raw_cnt, char* out, uint64_t cap, uint64_t* written);

/* Format and write many `.kf` files with n_threads host threads:
 * file i = dir + "/" + names[i] + ".kf", counts row i of counts[n x nbins]. */
int kf_write_kf_files(const char* dir, const char* const* names, int32_t n,
                      const uint32_t* counts, uint64_t nbins, int pseudocount,
                      int raw_cnt, int n_threads);

/* get_chunks (main.py:869-915): the rows of many windows in ONE file, in order:
 * path = the file, row i = names[i] + counts row i, formatted by n_threads host
 * threads (as kf_format_kf) and written in row order. */
int kf_write_kf_rows(const char* path, const char* const* names, int32_t n,
                     const uint32_t* counts, uint64_t nbins, int pseudocount,
                     int raw_cnt, int n_threads);

/* get_chunks, many genomes at once: segment g is rows [seg_row0[g],
 * seg_row0[g+1]) of counts (seg_row0[0] = 0, non-decreasing), written in row
 * order to paths[g] (distinct), appended if seg_append && seg_append[g] (a genome
 * whose windows span several count launches), else truncated.  Row i is named
 * names[i], or, with names == NULL, prefixes[row_prefix[i]] followed by
 * "<s+1>-<s+win_len>" for s = row_start[i] (the window names of main.py:905-915).
 * n_threads host threads format rows into private arenas and write each
 * segment's file once its rows are formatted (formatting and writing overlap). */
int kf_write_kf_segments(int32_t n_seg, const char* const* paths, const int32_t* seg_row0,
                         const uint8_t* seg_append, const char* const* names,
                         const char* const* prefixes, const uint32_t* row_prefix,
                         const uint64_t* row_start, uint32_t win_len,
                         const uint32_t* counts, uint64_t nbins, int pseudocount,
                         int raw_cnt, int n_threads);

/* kf_write_kf_segments for u16 counts (a get_chunks window of 10 kbp has every
 * count below 2^16, so its rows cross PCIe at half the bytes). */
int kf_write_kf_segments16(int32_t n_seg, const char* const* paths, const int32_t* seg_row0,
                           const uint8_t* seg_append, const char* const* names,
                           const char* const* prefixes, const uint32_t* row_prefix,
                           const uint64_t* row_start, uint32_t win_len,
                           const uint16_t* counts, uint64_t nbins, int pseudocount,
                           int raw_cnt, int n_threads);

/* get_chunks' writer of finished text (kf_format_kf_rows16's, once on the host):
 * segment g is text[seg_off[g], seg_off[g + 1]) (seg_off non-decreasing, n_seg +
 * 1 entries), written to paths[g] (distinct) from the file's start, truncating
 * it, or, if seg_append && seg_append[g], from its current end -- the meaning of
 * kf_write_kf_segments.  Nothing is formatted: blocks of 4 MiB are written with
 * pwrite at their file offsets by up to n_threads threads of the host pool.  An
 * empty segment still creates or truncates its file. */
int kf_write_text_segments(int32_t n_seg, const char* const* paths, const uint8_t* seg_append,
                           const uint64_t* seg_off, const uint8_t* text, int n_threads);

/* ---- get_chunks device pre-pass (replaces seqtk seq -l 0 | awk N-collapse |
 * seqkit seq -g -m, main.py:726-760).  d_seq holds n_rec sorted, disjoint
 * [start, end) byte ranges of record sequences (the bytes between a header's
 * '\n' and the next header); any such ranges do, cut mid-line or touching, but
 * every one must lie inside [0, len]: the bounds are clamped to len, the byte
 * rule is not (it reads d_bytes[j + 1] wherever j + 1 is below the range's
 * end).  Writes each record's processed sequence --
 * newlines and line-end '\r' dropped, the gap letters "- \t." dropped, runs of
 * N / n / '|' (awk runs before seqkit: gap letters split a run) collapsed to
 * one 'N' -- back to back into d_out (>= len bytes) and its [start, end) into
 * d_out_se[2r], d_out_se[2r+1].  d_scratch: >= ceil(len / 4096) + 1 words.
 * len < 2^32 (KF_EINVAL otherwise).  Asynchronous on `stream`. */
int kf_chunk_compact(const uint8_t* d_bytes, uint64_t len, const uint64_t* d_seq, int32_t n_rec,
                     uint8_t* d_out, uint64_t* d_out_se, uint32_t* d_scratch, uint64_t scratch_words,
                     void* stream);

/* Window w = d_src[d_win_src[w], + win_len) to d_dst[w * win_len, + win_len)
 * (the seqkit sliding windows of main.py:813-824, laid out for kf_count_batch). */
int kf_chunk_gather(const uint8_t* d_src, const uint64_t* d_win_src, int32_t n_win, uint32_t win_len,
                    uint8_t* d_dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KF2VEC_GPU_H */
