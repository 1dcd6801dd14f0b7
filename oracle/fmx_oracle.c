/*
 * fmx_oracle.c -- CPU restatement of findex's FM-index hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the product:
 * only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library, and there only as the checker / the timed CPU baseline.
 * The product (findex_amd/, libfmx.so) never links, imports or calls it.
 *
 * Parity status: PINNED BY FIXTURES.  The reference is Scala 2.10 on the JVM
 * and cannot be compiled or run in this image (no java/scala/sbt), so there is
 * no oracle/_ref build.  This restatement is pinned instead against every
 * known-answer and golden file the reference's own tests hold for this path
 * (see tests/test_oracle_kat.py, tests/golden/).  One thing stays unpinned:
 * the dequeue order among equal keys of scala.collection.mutable.PriorityQueue
 * (Scala 2.10.0), restated below from the published library source; no
 * reference test pins an outcome that depends on it.
 *
 * Every function cites the reference file:line it follows.  Paths are relative
 * to /root/reference:  F = src/main/scala/org/fmindex
 *
 * Positions are 64-bit here (the reference is Int/32-bit, F/findex.scala:10-13);
 * values are identical for n < 2^31.  The inverted list holds uint32 entries, so
 * this oracle supports n <= 2^32.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define ORC_OK 0
#define ORC_ERR_IO -1
#define ORC_ERR_FORMAT -2
#define ORC_ERR_INDEX -3   /* the reference would throw ArrayIndexOutOfBounds */
#define ORC_ERR_NOMEM -4
#define ORC_ERR_RANGE -5

#define ALPHA_SIZE 256     /* F/bwtmerger.scala BWTMerger2.ALPHA_SIZE, F/util.scala:91 */

typedef struct orc_index {
  uint64_t n;              /* rows incl. the EOF row = fm.size, F/bwtmerger.scala:339 */
  uint64_t eof;            /* BWT slot holding the EOF symbol, F/bwtmerger.scala:151 */
  uint8_t *bwt;            /* raw bytes as stored (slot eof is a filler byte) */
  int64_t aux[ALPHA_SIZE]; /* .aux counts, F/bwtmerger.scala:130-142 */
  uint64_t bs[ALPHA_SIZE];  /* bucketStarts : c2bs(aux with c(0):=1), F/bwtmerger.scala:346-350 */
  uint64_t bs0[ALPHA_SIZE]; /* bucketStarts0: c2bs(aux) untouched,    F/bwtmerger.scala:341-345 */
  uint32_t *fm;            /* inverted list = the .fm payload, F/bwtmerger.scala:424-533 */
} orc_index;

/* ---------------------------------------------------------------- formats */

static uint64_t rd_u64(const uint8_t *p, int big_endian) {
  uint64_t v = 0;
  if (big_endian) for (int i = 0; i < 8; i++) v = (v << 8) | p[i];
  else for (int i = 7; i >= 0; i--) v = (v << 8) | p[i];
  return v;
}

/* BWTLoader, F/bwtmerger.scala:144-174: int64 size, int64 eof, then size bytes;
 * size + 16 must equal the file length (:153). */
int orc_load_bwt(const char *path, int big_endian, uint8_t **bwt_out,
                 uint64_t *n_out, uint64_t *eof_out) {
  FILE *f = fopen(path, "rb");
  if (!f) return ORC_ERR_IO;
  uint8_t hdr[16];
  if (fread(hdr, 1, 16, f) != 16) { fclose(f); return ORC_ERR_FORMAT; }
  uint64_t size = rd_u64(hdr, big_endian), eof = rd_u64(hdr + 8, big_endian);
  fseek(f, 0, SEEK_END);
  uint64_t flen = (uint64_t)ftell(f);
  if (size + 16 != flen) { fclose(f); return ORC_ERR_FORMAT; }
  fseek(f, 16, SEEK_SET);
  uint8_t *b = (uint8_t *)malloc(size ? size : 1);
  if (!b) { fclose(f); return ORC_ERR_NOMEM; }
  if (fread(b, 1, size, f) != size) { free(b); fclose(f); return ORC_ERR_IO; }
  fclose(f);
  *bwt_out = b; *n_out = size; *eof_out = eof;
  return ORC_OK;
}

/* AUXLoader, F/bwtmerger.scala:130-142: exactly 256 int64 counts. */
int orc_load_aux(const char *path, int big_endian, int64_t aux[ALPHA_SIZE]) {
  FILE *f = fopen(path, "rb");
  if (!f) return ORC_ERR_IO;
  uint8_t buf[ALPHA_SIZE * 8];
  size_t got = fread(buf, 1, sizeof buf, f);
  fclose(f);
  if (got != sizeof buf) return ORC_ERR_FORMAT;
  for (int i = 0; i < ALPHA_SIZE; i++) aux[i] = (int64_t)rd_u64(buf + 8 * i, big_endian);
  return ORC_OK;
}

void orc_free_buf(void *p) { free(p); }

/* The .aux content for a BWT held in memory (AUXLoader's array, F/bwtmerger.scala:130-142): symbol counts
 * without the EOF slot, on `threads` cores -- bench.py needs it for multi-GiB synthetic BWTs. */
void orc_histogram(const uint8_t *bwt, uint64_t n, uint64_t eof, int threads, int64_t out[ALPHA_SIZE]) {
  if (threads < 1) threads = 1;
  int64_t *h = (int64_t *)calloc((size_t)threads * ALPHA_SIZE, sizeof(int64_t));
  const uint64_t chunk = (n + (uint64_t)threads - 1) / (uint64_t)threads;
#pragma omp parallel for num_threads(threads) schedule(static, 1)
  for (int t = 0; t < threads; t++) {
    uint64_t lo = chunk * (uint64_t)t, hi = lo + chunk;
    if (hi > n) hi = n;
    for (uint64_t i = lo; i < hi; i++) h[(size_t)t * ALPHA_SIZE + bwt[i]]++;
  }
  for (int c = 0; c < ALPHA_SIZE; c++) {
    out[c] = 0;
    for (int t = 0; t < threads; t++) out[c] += h[(size_t)t * ALPHA_SIZE + c];
  }
  if (eof < n) out[bwt[eof]]--;
  free(h);
}

/* ------------------------------------------------------------ construction */

/* c2bs, F/util.scala:109-119 */
static void c2bs(const int64_t c[ALPHA_SIZE], uint64_t bs[ALPHA_SIZE]) {
  uint64_t tot = 0;
  for (int i = 0; i < ALPHA_SIZE; i++) { bs[i] = tot; tot += (uint64_t)c[i]; }
}

/* FMCreator.create, F/bwtmerger.scala:452-532, in memory: a stable bucket sort
 * of BWT positions by symbol.  The byte at stream index eofNum is replaced by 0
 * (:493); bucket starts are bs(0)=0, bs(c)=1+sum_{1<=j<c} aux(j) (:440-450), i.e.
 * aux(0) is ignored and symbol 0 owns exactly the one EOF slot. */
static int build_fm(orc_index *ix) {
  uint64_t bkt[ALPHA_SIZE];
  uint64_t tot = 1;
  bkt[0] = 0;
  for (int i = 1; i < ALPHA_SIZE; i++) { bkt[i] = tot; tot += (uint64_t)ix->aux[i]; }
  ix->fm = (uint32_t *)malloc((ix->n ? ix->n : 1) * sizeof(uint32_t));
  if (!ix->fm) return ORC_ERR_NOMEM;
  uint64_t lim[ALPHA_SIZE];                       /* one past each bucket's last slot */
  for (int i = 0; i + 1 < ALPHA_SIZE; i++) lim[i] = bkt[i + 1];
  lim[ALPHA_SIZE - 1] = ix->n;
  for (uint64_t i = 0; i < ix->n; i++) {
    int c = (i == ix->eof) ? 0 : ix->bwt[i];
    /* a bucket overflow means .aux does not describe this .bwt; the reference
     * would silently write into the next bucket's file region */
    if (bkt[c] >= lim[c] || bkt[c] >= ix->n) return ORC_ERR_FORMAT;
    ix->fm[bkt[c]++] = (uint32_t)i;
  }
  return ORC_OK;
}

/* NaiveFMSearcher constructor, F/bwtmerger.scala:335-353 */
/* The same sort on `threads` cores (a 2^32-row list is built for bench.py's cpu_baseline): per-chunk symbol
 * histograms, prefix sums per symbol over the chunks, then every chunk scatters its own positions -- the result
 * is the stable order of build_fm.  Counts that do not match .aux are ORC_ERR_FORMAT as there. */
static int build_fm_mt(orc_index *ix, int threads) {
  if (threads < 2 || ix->n < (1u << 20)) return build_fm(ix);
  ix->fm = (uint32_t *)malloc(ix->n * sizeof(uint32_t));
  uint64_t *hist = (uint64_t *)calloc((size_t)threads * ALPHA_SIZE, sizeof(uint64_t));
  if (!ix->fm || !hist) { free(hist); return ORC_ERR_NOMEM; }
  const uint64_t chunk = (ix->n + (uint64_t)threads - 1) / (uint64_t)threads;
#pragma omp parallel for num_threads(threads) schedule(static, 1)
  for (int t = 0; t < threads; t++) {
    uint64_t lo = chunk * (uint64_t)t, hi = lo + chunk;
    if (hi > ix->n) hi = ix->n;
    uint64_t *h = hist + (size_t)t * ALPHA_SIZE;
    for (uint64_t i = lo; i < hi; i++) h[(i == ix->eof) ? 0 : ix->bwt[i]]++;
  }
  int rc = ORC_OK;
  uint64_t start = 0;
  for (int c = 0; c < ALPHA_SIZE; c++) {
    uint64_t tot = 0;
    for (int t = 0; t < threads; t++) { uint64_t v = hist[(size_t)t * ALPHA_SIZE + c]; hist[(size_t)t * ALPHA_SIZE + c] = start + tot; tot += v; }
    const uint64_t want = c == 0 ? 1 : (uint64_t)ix->aux[c];
    if (tot != want) rc = ORC_ERR_FORMAT;
    start += tot;
  }
  if (rc == ORC_OK) {
#pragma omp parallel for num_threads(threads) schedule(static, 1)
    for (int t = 0; t < threads; t++) {
      uint64_t lo = chunk * (uint64_t)t, hi = lo + chunk;
      if (hi > ix->n) hi = ix->n;
      uint64_t *h = hist + (size_t)t * ALPHA_SIZE;
      for (uint64_t i = lo; i < hi; i++) ix->fm[h[(i == ix->eof) ? 0 : ix->bwt[i]]++] = (uint32_t)i;
    }
  }
  free(hist);
  return rc;
}

static orc_index *open_mem_impl(const uint8_t *bwt, uint64_t n, uint64_t eof, const int64_t aux[ALPHA_SIZE],
                                int threads, int *err) {
  int e = ORC_OK;
  orc_index *ix = NULL;
  if (n > (1ull << 32) || eof >= (n ? n : 1)) { e = ORC_ERR_RANGE; goto done; }
  ix = (orc_index *)calloc(1, sizeof *ix);
  if (!ix) { e = ORC_ERR_NOMEM; goto done; }
  ix->n = n; ix->eof = eof;
  ix->bwt = (uint8_t *)malloc(n ? n : 1);
  if (!ix->bwt) { e = ORC_ERR_NOMEM; goto done; }
  memcpy(ix->bwt, bwt, n);
  memcpy(ix->aux, aux, sizeof ix->aux);
  int64_t c1[ALPHA_SIZE];
  memcpy(c1, aux, sizeof c1);
  c2bs(c1, ix->bs0);          /* :341-345 */
  c1[0] = 1;                  /* :348 */
  c2bs(c1, ix->bs);           /* :349 */
  e = build_fm_mt(ix, threads);
done:
  if (e != ORC_OK && ix) { free(ix->bwt); free(ix->fm); free(ix); ix = NULL; }
  if (err) *err = e;
  return ix;
}

orc_index *orc_open_mem(const uint8_t *bwt, uint64_t n, uint64_t eof, const int64_t aux[ALPHA_SIZE], int *err) {
  return open_mem_impl(bwt, n, eof, aux, 1, err);
}
orc_index *orc_open_mem_threads(const uint8_t *bwt, uint64_t n, uint64_t eof, const int64_t aux[ALPHA_SIZE],
                                int threads, int *err) {
  return open_mem_impl(bwt, n, eof, aux, threads, err);
}

orc_index *orc_open_files(const char *bwt_path, const char *aux_path, int big_endian, int *err) {
  uint8_t *bwt = NULL; uint64_t n = 0, eof = 0; int64_t aux[ALPHA_SIZE];
  int e = orc_load_bwt(bwt_path, big_endian, &bwt, &n, &eof);
  if (e == ORC_OK) e = orc_load_aux(aux_path, big_endian, aux);
  orc_index *ix = NULL;
  if (e == ORC_OK) ix = orc_open_mem(bwt, n, eof, aux, &e);
  free(bwt);
  if (err) *err = e;
  return ix;
}

void orc_close(orc_index *ix) {
  if (!ix) return;
  free(ix->bwt); free(ix->fm); free(ix);
}

uint64_t orc_n(const orc_index *ix) { return ix->n; }
uint64_t orc_eof(const orc_index *ix) { return ix->eof; }
const uint32_t *orc_fm_ptr(const orc_index *ix) { return ix->fm; }
const uint8_t *orc_bwt_ptr(const orc_index *ix) { return ix->bwt; }

/* .fm wire format, F/bwtmerger.scala:483-485,476-481: byte elSize(=4), int64 BE
 * size, then size x int32 BE. */
int orc_write_fm(const orc_index *ix, const char *path) {
  FILE *f = fopen(path, "wb");
  if (!f) return ORC_ERR_IO;
  uint8_t hdr[9];
  hdr[0] = 4;
  for (int i = 0; i < 8; i++) hdr[1 + i] = (uint8_t)(ix->n >> (56 - 8 * i));
  fwrite(hdr, 1, 9, f);
  for (uint64_t i = 0; i < ix->n; i++) {
    uint32_t v = ix->fm[i];
    uint8_t b[4] = {(uint8_t)(v >> 24), (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v};
    fwrite(b, 1, 4, f);
  }
  fclose(f);
  return ORC_OK;
}

/* --------------------------------------------------------------- rank / LF */

/* NaiveFMSearcher.cf, F/bwtmerger.scala:352 */
int64_t orc_cf(const orc_index *ix, int c) {
  if (c < 0 || c >= ALPHA_SIZE) return ORC_ERR_INDEX;
  return (int64_t)ix->bs[c];
}

/* NaiveFMSearcher.occ, F/bwtmerger.scala:354-375: binary search for `key` in
 * fm[bs(c) .. bs(c+1)-1] (last bucket ends at n-1); number of entries <= key. */
int64_t orc_occ(const orc_index *ix, int c, int64_t key) {
  if (c < 0 || c >= ALPHA_SIZE) return ORC_ERR_INDEX;
  int64_t istart = (int64_t)ix->bs[c];
  int64_t imin = istart;
  int64_t imax = (c == ALPHA_SIZE - 1) ? (int64_t)ix->n - 1 : (int64_t)ix->bs[c + 1] - 1;
  if (imin <= imax) {
    int found = 0;
    int64_t imid = 0, ival = 0;
    while (!found && imax >= imin) {
      imid = (imax + imin) / 2;
      ival = (int64_t)ix->fm[imid];
      if (ival < key) imin = imid + 1;
      else if (ival > key) imax = imid - 1;
      else found = 1;
    }
    return (ival <= key) ? (imid - istart + 1) : (imid - istart);
  }
  return 0;
}

/* SuffixAlgo.search, F/findex.scala:15-31.  Returns 1 for Some((sp,ep)), 0 for
 * None; sp/ep always receive the loop's final values.  The reference indexes
 * cf/occ with a signed Byte, so bytes >= 0x80 throw (F/findex.scala:21,26):
 * strict_signed=1 reports that as ORC_ERR_INDEX; 0 reads the byte unsigned
 * (the product's documented superset).  *steps = loop iterations executed. */
int orc_search(const orc_index *ix, const uint8_t *in, uint64_t len, int strict_signed,
               uint64_t *sp_out, uint64_t *ep_out, uint32_t *steps) {
  int64_t sp = 0, ep = (int64_t)ix->n;
  int64_t i = (int64_t)len - 1;
  uint32_t st = 0;
  while (sp < ep && i >= 0) {
    int c = in[i];
    if (strict_signed && c >= 0x80) return ORC_ERR_INDEX;
    i -= 1;
    int64_t nsp = orc_cf(ix, c) + orc_occ(ix, c, sp - 1);
    int64_t nep = orc_cf(ix, c) + orc_occ(ix, c, ep - 1);
    sp = nsp; ep = nep;
    st++;
  }
  *sp_out = (uint64_t)sp; *ep_out = (uint64_t)ep;
  if (steps) *steps = st;
  return sp < ep ? 1 : 0;
}

/* SuffixAlgo.getPrevRange, F/findex.scala:32-36 */
int orc_get_prev_range(const orc_index *ix, int64_t sp, int64_t ep, int c,
                       uint64_t *sp1, uint64_t *ep1) {
  if (c < 0 || c >= ALPHA_SIZE) return ORC_ERR_INDEX;
  int64_t a = orc_cf(ix, c) + orc_occ(ix, c, sp - 1);
  int64_t b = orc_cf(ix, c) + orc_occ(ix, c, ep - 1);
  *sp1 = (uint64_t)a; *ep1 = (uint64_t)b;
  return a < b ? 1 : 0;
}

/* SuffixAlgo.getIntervalPrevRange, F/findex.scala:37-51: every c in
 * [cstart,cend] inclusive; non-empty ranges only; the Scala list is built by
 * prepending, so it comes back in DESCENDING c.  out arrays need room for
 * cend-cstart+1 entries.  Returns the number of ranges or ORC_ERR_INDEX. */
int orc_get_interval_prev_range(const orc_index *ix, int64_t sp, int64_t ep, int cstart, int cend,
                                uint64_t *out_sp, uint64_t *out_ep, int *out_c) {
  if (cstart < 0 || (cstart <= cend && cend >= ALPHA_SIZE)) return ORC_ERR_INDEX;
  int k = 0;
  for (int c = cstart; c <= cend; c++) {
    int64_t occ1 = orc_occ(ix, c, sp - 1), occ2 = orc_occ(ix, c, ep - 1);
    if (occ1 < occ2) {
      out_sp[k] = (uint64_t)(orc_cf(ix, c) + occ1);
      out_ep[k] = (uint64_t)(orc_cf(ix, c) + occ2);
      if (out_c) out_c[k] = c;
      k++;
    }
  }
  for (int a = 0, b = k - 1; a < b; a++, b--) {   /* prepend order */
    uint64_t t = out_sp[a]; out_sp[a] = out_sp[b]; out_sp[b] = t;
    t = out_ep[a]; out_ep[a] = out_ep[b]; out_ep[b] = t;
    if (out_c) { int tc = out_c[a]; out_c[a] = out_c[b]; out_c[b] = tc; }
  }
  return k;
}

/* BWTLoader.read, F/bwtmerger.scala:155-162: 0 at i == eof */
static int bwt_read(const orc_index *ix, uint64_t i) { return i == ix->eof ? 0 : ix->bwt[i]; }
int orc_bwt_read(const orc_index *ix, uint64_t i) { return i < ix->n ? bwt_read(ix, i) : ORC_ERR_INDEX; }

/* NaiveFMSearcher.pos2char, F/bwtmerger.scala:376-385 (uses bucketStarts0) */
int orc_pos2char(const orc_index *ix, int64_t key) {
  int i = ALPHA_SIZE - 1;
  if ((int64_t)ix->bs0[i] > key) {
    while ((int64_t)ix->bs0[i] > key && i > 0) i -= 1;
  } else {
    while (ix->bs0[i - 1] == ix->bs0[i] && i > 1) i -= 1;
    i -= 1;
  }
  return i;
}

/* NaiveFMSearcher.getPrevI (LF step), F/bwtmerger.scala:386-389 */
int64_t orc_get_prev_i(const orc_index *ix, int64_t i) {
  if (i < 0 || (uint64_t)i >= ix->n) return ORC_ERR_INDEX;
  int c = bwt_read(ix, (uint64_t)i);
  return orc_cf(ix, c) + orc_occ(ix, c, i - 1);
}

/* NaiveFMSearcher.getNextI (Psi step), F/bwtmerger.scala:390-392 */
int64_t orc_get_next_i(const orc_index *ix, int64_t i) {
  if (i < 0 || (uint64_t)i >= ix->n) return ORC_ERR_INDEX;
  return (int64_t)ix->fm[i];
}

/* NaiveFMSearcher.nextSubstr, F/bwtmerger.scala:394-405: walk Psi, stop after
 * appending a 0 byte, then reverse.  Returns the number of bytes written. */
int64_t orc_next_substr(const orc_index *ix, int64_t sp, int64_t len, uint8_t *out) {
  if (sp < 0 || (uint64_t)sp >= ix->n) return ORC_ERR_INDEX;
  int64_t cp = orc_get_next_i(ix, sp), k = 0;
  int eof = 0;
  for (int64_t i = 0; i < len && !eof; i++) {
    int b = bwt_read(ix, (uint64_t)cp);
    eof = (b == 0);
    out[k++] = (uint8_t)b;
    cp = orc_get_next_i(ix, cp);
  }
  for (int64_t a = 0, b = k - 1; a < b; a++, b--) { uint8_t t = out[a]; out[a] = out[b]; out[b] = t; }
  return k;
}

/* NaiveFMSearcher.prevSubstr, F/bwtmerger.scala:409-419: walk LF; `eof` is
 * never set there, so the walk runs through the EOF row for all len steps. */
int64_t orc_prev_substr(const orc_index *ix, int64_t sp, int64_t len, uint8_t *out) {
  if (sp < 0 || (uint64_t)sp >= ix->n) return ORC_ERR_INDEX;
  int64_t cp = sp;
  for (int64_t i = 0; i < len; i++) {
    out[i] = (uint8_t)bwt_read(ix, (uint64_t)cp);
    cp = orc_get_prev_i(ix, cp);
  }
  return len;
}

/* ----------------------------------------------------------------- batches */
/* Plain loops over the functions above; `threads` > 1 uses OpenMP when built
 * with -fopenmp (bench.py's cpu_baseline leg). */

/* One dependent chain of `steps` rank steps, curRank = cf(c) + occ(c, curRank - 1), the shape of BWTMerger2.calcGaps'
 * inner loop (F/bwtmerger.scala:992-999; there c comes from the already-merged text, here from the BWT itself, i.e. an
 * LF walk).  Timed by tools/calcgaps_chain.py beside the same chain on the GPU. */
int64_t orc_lf_chain(const orc_index *ix, int64_t row, int64_t steps) {
  for (int64_t s = 0; s < steps; s++) {
    const int c = bwt_read(ix, (uint64_t)row);
    row = (int64_t)ix->bs[c] + orc_occ(ix, c, row - 1);
  }
  return row;
}

/* calcGaps' own chain over a given text (F/bwtmerger.scala:999-1001, without the lastChar correction):
 * curRank = cFirst if curRank == 0 else cFirst + occ(c, curRank - 1); ranks[j] = curRank after byte j. */
int orc_occ_chain(const orc_index *ix, const uint8_t *c, uint64_t k, int64_t rank0, int64_t *ranks) {
  int64_t cur = rank0;
  for (uint64_t j = 0; j < k; j++) {
    cur = (int64_t)ix->bs[c[j]] + (cur == 0 ? 0 : orc_occ(ix, c[j], cur - 1));
    ranks[j] = cur;
  }
  return ORC_OK;
}

int orc_occ_batch(const orc_index *ix, const uint8_t *c, const int64_t *i, int64_t *out, uint64_t k) {
  for (uint64_t q = 0; q < k; q++) out[q] = orc_occ(ix, c[q], i[q]);
  return ORC_OK;
}

int orc_search_batch(const orc_index *ix, const uint8_t *pat, const uint64_t *off, uint64_t k,
                     uint64_t *sp, uint64_t *ep, uint32_t *steps, int threads) {
  int bad = 0;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 256) num_threads(threads > 0 ? threads : 1)
#endif
  for (int64_t q = 0; q < (int64_t)k; q++) {
    uint32_t st = 0;
    int r = orc_search(ix, pat + off[q], off[q + 1] - off[q], 0, &sp[q], &ep[q], &st);
    if (steps) steps[q] = st;
    if (r < 0) bad = 1;
  }
  (void)threads;
  return bad ? ORC_ERR_INDEX : ORC_OK;
}

int orc_prev_range_batch(const orc_index *ix, const uint64_t *sp, const uint64_t *ep, const uint8_t *c,
                         uint64_t *sp1, uint64_t *ep1, uint64_t k) {
  for (uint64_t q = 0; q < k; q++) orc_get_prev_range(ix, (int64_t)sp[q], (int64_t)ep[q], c[q], &sp1[q], &ep1[q]);
  return ORC_OK;
}

/* -------------------------------------------------- Glushkov frontier search */
/* ReTree._matchSA, F/re2/retree.scala:618-653, over tables produced by the
 * Python restatement of ReTree (oracle/retree.py): per CharNode its byte `c`,
 * `num` (F/re2/retree.scala:393-423), `isLast` (:40-50) and `follows` (:14-38)
 * as a CSR list that keeps the reference's order and multiplicity. */

typedef struct { int64_t len; int64_t sp, ep; int32_t state; } orc_sp;   /* StatePoint :562 */

typedef struct { orc_sp *a; int64_t size0, cap; const int32_t *num; } orc_pq;

/* StatePoint.compare, F/re2/retree.scala:564: this < that  <=>  this.num > that.num */
static int pq_lt(const orc_pq *q, const orc_sp *x, const orc_sp *y) { return q->num[x->state] > q->num[y->state]; }

/* scala.collection.mutable.PriorityQueue (Scala 2.10.0): a 1-based binary heap
 * in a resizable array; `+=` appends then fixUp, `dequeue` swaps the root with
 * the last slot and fixDown-s.  Restated from the library source. */
static int pq_push(orc_pq *q, orc_sp e) {
  if (q->size0 + 1 > q->cap) {
    int64_t nc = q->cap ? q->cap * 2 : 64;
    orc_sp *na = (orc_sp *)realloc(q->a, (size_t)nc * sizeof(orc_sp));
    if (!na) return ORC_ERR_NOMEM;
    q->a = na; q->cap = nc;
  }
  q->a[q->size0] = e;
  int64_t k = q->size0;                          /* fixUp(as, size0) */
  while (k > 1 && pq_lt(q, &q->a[k / 2], &q->a[k])) {
    orc_sp t = q->a[k]; q->a[k] = q->a[k / 2]; q->a[k / 2] = t;
    k = k / 2;
  }
  q->size0 += 1;
  return ORC_OK;
}

static orc_sp pq_pop(orc_pq *q) {
  q->size0 -= 1;
  orc_sp t = q->a[1]; q->a[1] = q->a[q->size0]; q->a[q->size0] = t;
  int64_t n = q->size0 - 1, k = 1;               /* fixDown(as, 1, size0-1) */
  while (n >= 2 * k) {
    int64_t j = 2 * k;
    if (j < n && pq_lt(q, &q->a[j], &q->a[j + 1])) j += 1;
    if (!pq_lt(q, &q->a[k], &q->a[j])) break;    /* as(k) >= as(j) */
    orc_sp h = q->a[k]; q->a[k] = q->a[j]; q->a[j] = h;
    k = j;
  }
  return q->a[q->size0];
}

/* Returns the number of results (written newest-first, i.e. in the reference's
 * `ret ::= ...` list order, up to cap) or a negative error.  *front_left = size
 * of the leftover frontier, *pops = getPrevRange calls made.
 * matchSA itself (F/re2/retree.scala:570-617) returns this first-pass `ret`
 * whatever the exploratory restarts at :578-614 find, so they are not restated. */
/* max_len > 0 caps the match length like the product's fmx_limits.max_steps (a bench / test variant, not in the
 * reference): a popped element whose children would have len >= max_len is not expanded; *truncated says so. */
static int64_t match_sa_core(const orc_index *ix, int32_t nstates, const uint8_t *st_c, const int32_t *st_num,
                             const uint8_t *st_last, const int32_t *fol_off, const int32_t *fol,
                             const int32_t *firsts, int32_t nfirsts, int64_t max_branching, int64_t max_iterations,
                             int64_t max_len, int64_t *res_len, uint64_t *res_sp, uint64_t *res_ep, int64_t cap,
                             int64_t *front_left, int64_t *pops, int *truncated) {
  (void)nstates;
  orc_pq q = {0};
  q.num = st_num;
  q.size0 = 1;                                   /* array(0) is unused */
  q.cap = 0;
  /* discovery-ordered scratch; reversed into the output at the end */
  int64_t nres = 0, rcap = 1024;
  int64_t *rl = (int64_t *)malloc((size_t)rcap * sizeof(int64_t));
  uint64_t *rs = (uint64_t *)malloc((size_t)rcap * sizeof(uint64_t));
  uint64_t *re = (uint64_t *)malloc((size_t)rcap * sizeof(uint64_t));
  int64_t rc = ORC_OK;
  for (int32_t f = 0; f < nfirsts; f++) {        /* pqFront ++= inputStates, :624 */
    orc_sp e = {0, 0, (int64_t)ix->n, firsts[f]};
    if (pq_push(&q, e) != ORC_OK) { rc = ORC_ERR_NOMEM; goto out; }
  }
  int64_t i = 1, npop = 0;
  while (q.size0 >= 2 && (q.size0 - 1) < max_branching && (max_iterations == 0 || i < max_iterations)) {  /* :628 */
    orc_sp s = pq_pop(&q);
    uint64_t sp1, ep1;
    npop++;
    if (orc_get_prev_range(ix, s.sp, s.ep, st_c[s.state], &sp1, &ep1) == 1) {   /* :633 */
      if (st_last[s.state]) {                                                  /* :636-638 */
        if (nres == rcap) {
          rcap *= 2;
          rl = (int64_t *)realloc(rl, (size_t)rcap * sizeof(int64_t));
          rs = (uint64_t *)realloc(rs, (size_t)rcap * sizeof(uint64_t));
          re = (uint64_t *)realloc(re, (size_t)rcap * sizeof(uint64_t));
          if (!rl || !rs || !re) { rc = ORC_ERR_NOMEM; goto out; }
        }
        rl[nres] = s.len + 1; rs[nres] = sp1; re[nres] = ep1; nres++;
      } else if (max_len > 0 && s.len + 1 >= max_len) {
        if (truncated && fol_off[s.state + 1] > fol_off[s.state]) *truncated = 1;
      } else {                                                                 /* :641 */
        for (int32_t j = fol_off[s.state]; j < fol_off[s.state + 1]; j++) {
          orc_sp e = {s.len + 1, (int64_t)sp1, (int64_t)ep1, fol[j]};
          if (pq_push(&q, e) != ORC_OK) { rc = ORC_ERR_NOMEM; goto out; }
        }
      }
    }
    i += 1;
  }
  if (front_left) *front_left = q.size0 - 1;
  if (pops) *pops = npop;
  for (int64_t k = 0; k < nres && k < cap; k++) {          /* newest first */
    res_len[k] = rl[nres - 1 - k]; res_sp[k] = rs[nres - 1 - k]; res_ep[k] = re[nres - 1 - k];
  }
  rc = nres;
out:
  free(q.a); free(rl); free(rs); free(re);
  return rc;
}

/* ReTree._matchSA, F/re2/retree.scala:618-653 (the reference's own loop, limits and pop order). */
int64_t orc_match_sa(const orc_index *ix, int32_t nstates, const uint8_t *st_c, const int32_t *st_num,
                     const uint8_t *st_last, const int32_t *fol_off, const int32_t *fol,
                     const int32_t *firsts, int32_t nfirsts, int64_t max_branching, int64_t max_iterations,
                     int64_t *res_len, uint64_t *res_sp, uint64_t *res_ep, int64_t cap,
                     int64_t *front_left, int64_t *pops) {
  return match_sa_core(ix, nstates, st_c, st_num, st_last, fol_off, fol, firsts, nfirsts, max_branching,
                       max_iterations, 0, res_len, res_sp, res_ep, cap, front_left, pops, NULL);
}

/* The same over a batch of regexes on `threads` host cores (bench.py's cpu_baseline for the regex workload and
 * full-size parity checks): regex r has states st_off[r] .. st_off[r+1] of the concatenated st_* arrays, its
 * follows CSR (ns_r + 1 offsets, local state ids) at fol_off + st_off[r] + r with entries from fol + fol_base[r],
 * and its firsts at firsts + first_off[r].  Results land in out_* grouped by regex, each group sorted by
 * (len, sp, ep) -- the product's frontier-mode order; res_start gets k + 1 offsets.  Returns the number of results
 * (more than cap: nothing was written), or a negative error.  *pops_total = getPrevRange calls made. */
typedef struct { int64_t len; uint64_t sp, ep; } orc_res;
static int res_cmp(const void *a, const void *b) {
  const orc_res *x = (const orc_res *)a, *y = (const orc_res *)b;
  if (x->len != y->len) return x->len < y->len ? -1 : 1;
  if (x->sp != y->sp) return x->sp < y->sp ? -1 : 1;
  if (x->ep != y->ep) return x->ep < y->ep ? -1 : 1;
  return 0;
}
static int64_t match_sa_batch_impl(const orc_index *ix, int64_t k, const int64_t *st_off, const uint8_t *st_c,
                           const int32_t *st_num, const uint8_t *st_last, const int32_t *fol_off,
                           const int64_t *fol_base, const int32_t *fol, const int64_t *first_off,
                           const int32_t *firsts, int64_t max_branching, int64_t max_iterations, int64_t max_len,
                           int threads, int64_t *res_start, int64_t *out_len, uint64_t *out_sp, uint64_t *out_ep,
                           int64_t cap, int64_t *pops_total, int64_t *n_truncated, int sorted) {
  orc_res **per = (orc_res **)calloc((size_t)(k ? k : 1), sizeof(orc_res *));
  int64_t *cnt = (int64_t *)calloc((size_t)(k ? k : 1), sizeof(int64_t));
  if (!per || !cnt) { free(per); free(cnt); return ORC_ERR_NOMEM; }
  int64_t pops_sum = 0, trunc_sum = 0, bad = 0;
  if (threads < 1) threads = 1;
#pragma omp parallel for schedule(dynamic, 16) num_threads(threads) reduction(+ : pops_sum, trunc_sum, bad)
  for (int64_t r = 0; r < k; r++) {
    const int64_t s0 = st_off[r];
    const int32_t ns = (int32_t)(st_off[r + 1] - s0);
    int64_t rcap = 64, got;
    int64_t *rl = NULL; uint64_t *rs = NULL, *re = NULL;
    int64_t left = 0, pops = 0;
    int trunc = 0;
    for (;;) {      /* grow until the regex's results fit */
      rl = (int64_t *)malloc((size_t)rcap * sizeof(int64_t));
      rs = (uint64_t *)malloc((size_t)rcap * sizeof(uint64_t));
      re = (uint64_t *)malloc((size_t)rcap * sizeof(uint64_t));
      if (!rl || !rs || !re) { got = ORC_ERR_NOMEM; break; }
      trunc = 0;
      got = match_sa_core(ix, ns, st_c + s0, st_num + s0, st_last + s0, fol_off + s0 + r, fol + fol_base[r],
                          firsts + first_off[r], (int32_t)(first_off[r + 1] - first_off[r]), max_branching,
                          max_iterations, max_len, rl, rs, re, rcap, &left, &pops, &trunc);
      if (got <= rcap) break;
      free(rl); free(rs); free(re);
      rcap = got;
    }
    if (got < 0) { bad++; free(rl); free(rs); free(re); continue; }
    pops_sum += pops;
    trunc_sum += trunc;
    cnt[r] = got;
    if (got) {
      per[r] = (orc_res *)malloc((size_t)got * sizeof(orc_res));
      if (!per[r]) { bad++; cnt[r] = 0; }
      else {
        for (int64_t j = 0; j < got; j++) { per[r][j].len = rl[j]; per[r][j].sp = rs[j]; per[r][j].ep = re[j]; }
        if (sorted) qsort(per[r], (size_t)got, sizeof(orc_res), res_cmp);
      }
    }
    free(rl); free(rs); free(re);
  }
  int64_t total = 0;
  for (int64_t r = 0; r < k; r++) { res_start[r] = total; total += cnt[r]; }
  res_start[k] = total;
  if (!bad && total <= cap)
    for (int64_t r = 0; r < k; r++)
      for (int64_t j = 0; j < cnt[r]; j++) {
        out_len[res_start[r] + j] = per[r][j].len;
        out_sp[res_start[r] + j] = per[r][j].sp;
        out_ep[res_start[r] + j] = per[r][j].ep;
      }
  for (int64_t r = 0; r < k; r++) free(per[r]);
  free(per); free(cnt);
  if (pops_total) *pops_total = pops_sum;
  if (n_truncated) *n_truncated = trunc_sum;
  return bad ? ORC_ERR_NOMEM : total;
}

/* per regex sorted by (len, sp, ep): the form results are compared in while the limits do not bind */
int64_t orc_match_sa_batch(const orc_index *ix, int64_t k, const int64_t *st_off, const uint8_t *st_c,
                           const int32_t *st_num, const uint8_t *st_last, const int32_t *fol_off,
                           const int64_t *fol_base, const int32_t *fol, const int64_t *first_off,
                           const int32_t *firsts, int64_t max_branching, int64_t max_iterations, int64_t max_len,
                           int threads, int64_t *res_start, int64_t *out_len, uint64_t *out_sp, uint64_t *out_ep,
                           int64_t cap, int64_t *pops_total, int64_t *n_truncated) {
  return match_sa_batch_impl(ix, k, st_off, st_c, st_num, st_last, fol_off, fol_base, fol, first_off, firsts, max_branching,
                             max_iterations, max_len, threads, res_start, out_len, out_sp, out_ep, cap, pops_total,
                             n_truncated, 1);
}

/* per regex in the reference's own list order (`ret ::= ...`, newest first, retree.scala:638): what
 * ReTree.matchSA returns under binding limits */
int64_t orc_match_sa_batch_ordered(const orc_index *ix, int64_t k, const int64_t *st_off, const uint8_t *st_c,
                           const int32_t *st_num, const uint8_t *st_last, const int32_t *fol_off,
                           const int64_t *fol_base, const int32_t *fol, const int64_t *first_off,
                           const int32_t *firsts, int64_t max_branching, int64_t max_iterations, int64_t max_len,
                           int threads, int64_t *res_start, int64_t *out_len, uint64_t *out_sp, uint64_t *out_ep,
                           int64_t cap, int64_t *pops_total, int64_t *n_truncated) {
  return match_sa_batch_impl(ix, k, st_off, st_c, st_num, st_last, fol_off, fol_base, fol, first_off, firsts, max_branching,
                             max_iterations, max_len, threads, res_start, out_len, out_sp, out_ep, cap, pops_total,
                             n_truncated, 0);
}

/* ------------------------------------------------------------------------------------------------------------------
 * Sampled-checkpoint variant of occ, for indexes the inverted lists cannot describe (n > 2^32: uint32 entries; or 6 n bytes
 * of host memory that are not there).  BASELINE.md ("CPU-baseline plan", n >= 2^31): "if host RAM cannot hold it, the CPU
 * baseline switches to a sampled popcount structure and the report says so".  NOT the reference's data structure -- the
 * reference binary-searches the .fm lists (F/bwtmerger.scala:354-375) -- but the same function: occ(c, i) = #{p <= i :
 * BWT'[p] == c} with BWT' = the BWT with slot eof read as symbol 0, cf(c) = NaiveFMSearcher.bucketStarts (:346-350), and the
 * reference's own search loop on top (F/findex.scala:15-31).  tests/test_oracle_kat.py holds it to the inverted-list oracle
 * on every fixture file and on random indexes.
 *   chk[b * nslots + s] = occurrences of the s-th present symbol in BWT'[0 .. 256 b)          (uint32: every count < 2^32)
 *   occ(c, i) = chk[(i + 1) / 256][slot(c)] + #{p in [256 * ((i + 1) / 256), i] : BWT'[p] == c}
 * 4 * nslots / 256 bytes per row beside the BWT itself: n = 2^34, sigma = 128 -> 32 GiB + 16 GiB. */
typedef struct orc_sampled {
  uint64_t n, eof, nblocks;
  const uint8_t *bwt;        /* the caller's bytes (kept alive by the caller); slot eof is read as 0 */
  uint32_t nslots;
  int16_t slot[ALPHA_SIZE];  /* symbol -> dense slot, -1: does not occur */
  uint64_t bs[ALPHA_SIZE];   /* bucketStarts, F/bwtmerger.scala:346-350 */
  uint32_t *chk;
} orc_sampled;

void orc_sampled_close(orc_sampled *s) {
  if (!s) return;
  free(s->chk);
  free(s);
}

orc_sampled *orc_sampled_open(const uint8_t *bwt, uint64_t n, uint64_t eof, int threads, int *err) {
  *err = ORC_OK;
  if (n < 1 || eof >= n) { *err = ORC_ERR_RANGE; return NULL; }
  orc_sampled *s = calloc(1, sizeof *s);
  if (!s) { *err = ORC_ERR_NOMEM; return NULL; }
  s->n = n; s->eof = eof; s->bwt = bwt;
  s->nblocks = n / 256 + 1;
  /* pass 1: per-chunk histograms of BWT' (the chunks are whole blocks) */
  const uint64_t chunk_blocks = 1u << 12;                       /* 1 Mi positions per chunk */
  const uint64_t nchunks = (s->nblocks + chunk_blocks - 1) / chunk_blocks;
  uint64_t *hist = calloc(nchunks * ALPHA_SIZE, sizeof(uint64_t));
  if (!hist) { orc_sampled_close(s); *err = ORC_ERR_NOMEM; return NULL; }
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 4) num_threads(threads > 0 ? threads : 1)
#endif
  for (int64_t ch = 0; ch < (int64_t)nchunks; ch++) {
    uint64_t a = (uint64_t)ch * chunk_blocks * 256, b = a + chunk_blocks * 256;
    if (b > n) b = n;
    uint64_t *h = hist + (uint64_t)ch * ALPHA_SIZE;
    for (uint64_t p = a; p < b; p++) h[p == eof ? 0 : bwt[p]]++;
  }
  int64_t total[ALPHA_SIZE];
  memset(total, 0, sizeof total);
  for (uint64_t ch = 0; ch < nchunks; ch++)
    for (int c = 0; c < ALPHA_SIZE; c++) total[c] += (int64_t)hist[ch * ALPHA_SIZE + c];
  for (int c = 0; c < ALPHA_SIZE; c++) {
    s->slot[c] = -1;
    if (total[c] > 0) {
      if ((uint64_t)total[c] >= (1ull << 32)) { free(hist); orc_sampled_close(s); *err = ORC_ERR_RANGE; return NULL; }
      s->slot[c] = (int16_t)s->nslots++;
    }
  }
  {   /* bucketStarts = c2bs(aux with c(0) := 1): cf(0) = 0, cf(c) = 1 + sum_{1 <= j < c} aux[j]; aux = the counts without the EOF symbol */
    int64_t aux[ALPHA_SIZE];
    for (int c = 0; c < ALPHA_SIZE; c++) aux[c] = total[c];
    aux[0] = 1;
    c2bs(aux, s->bs);
  }
  s->chk = malloc(s->nblocks * (uint64_t)s->nslots * sizeof(uint32_t));
  if (!s->chk) { free(hist); orc_sampled_close(s); *err = ORC_ERR_NOMEM; return NULL; }
  /* chunk prefix sums, then pass 2: every chunk fills its blocks' checkpoints from its own start */
  uint64_t run[ALPHA_SIZE];
  memset(run, 0, sizeof run);
  for (uint64_t ch = 0; ch < nchunks; ch++)
    for (int c = 0; c < ALPHA_SIZE; c++) { const uint64_t v = hist[ch * ALPHA_SIZE + c]; hist[ch * ALPHA_SIZE + c] = run[c]; run[c] += v; }
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 4) num_threads(threads > 0 ? threads : 1)
#endif
  for (int64_t ch = 0; ch < (int64_t)nchunks; ch++) {
    uint32_t cnt[ALPHA_SIZE];
    for (int c = 0; c < ALPHA_SIZE; c++) cnt[c] = (uint32_t)hist[(uint64_t)ch * ALPHA_SIZE + c];
    uint64_t b0 = (uint64_t)ch * chunk_blocks, b1 = b0 + chunk_blocks;
    if (b1 > s->nblocks) b1 = s->nblocks;
    for (uint64_t b = b0; b < b1; b++) {
      uint32_t *row = s->chk + b * s->nslots;
      for (int c = 0; c < ALPHA_SIZE; c++) if (s->slot[c] >= 0) row[s->slot[c]] = cnt[c];
      uint64_t a = b * 256, e = a + 256;
      if (e > n) e = n;
      for (uint64_t p = a; p < e; p++) cnt[p == eof ? 0 : bwt[p]]++;
    }
  }
  free(hist);
  return s;
}

uint64_t orc_sampled_bytes(const orc_sampled *s) { return s->nblocks * (uint64_t)s->nslots * sizeof(uint32_t); }

/* NaiveFMSearcher.occ's VALUE (F/bwtmerger.scala:354-375): #{p <= key : BWT'[p] == c}; key < 0 -> 0, key >= n clamps */
static int64_t sampled_occ(const orc_sampled *s, int c, int64_t key) {
  if (key < 0 || s->slot[c] < 0) return 0;
  uint64_t x = (uint64_t)key + 1;                 /* positions [0, x) */
  if (x > s->n) x = s->n;
  const uint64_t b = x >> 8;
  int64_t r = s->chk[b * s->nslots + (uint32_t)s->slot[c]];
  for (uint64_t p = b << 8; p < x; p++) r += (p == s->eof ? 0 : s->bwt[p]) == c;
  return r;
}
int64_t orc_sampled_occ(const orc_sampled *s, int c, int64_t key) { return (c < 0 || c > 255) ? ORC_ERR_INDEX : sampled_occ(s, c, key); }
int64_t orc_sampled_cf(const orc_sampled *s, int c) { return (c < 0 || c > 255) ? ORC_ERR_INDEX : (int64_t)s->bs[c]; }

/* SuffixAlgo.search, F/findex.scala:15-31, over the sampled occ (bytes read unsigned, like orc_search with strict_signed = 0) */
int orc_sampled_search_batch(const orc_sampled *s, const uint8_t *pat, const uint64_t *off, uint64_t k,
                             uint64_t *sp_out, uint64_t *ep_out, uint32_t *steps, int threads) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 256) num_threads(threads > 0 ? threads : 1)
#endif
  for (int64_t q = 0; q < (int64_t)k; q++) {
    const uint8_t *in = pat + off[q];
    int64_t sp = 0, ep = (int64_t)s->n, i = (int64_t)(off[q + 1] - off[q]) - 1;
    uint32_t st = 0;
    while (sp < ep && i >= 0) {
      const int c = in[i];
      i -= 1;
      const int64_t nsp = (int64_t)s->bs[c] + sampled_occ(s, c, sp - 1);
      const int64_t nep = (int64_t)s->bs[c] + sampled_occ(s, c, ep - 1);
      sp = nsp; ep = nep;
      st++;
    }
    sp_out[q] = (uint64_t)sp; ep_out[q] = (uint64_t)ep;
    if (steps) steps[q] = st;
  }
  (void)threads;
  return ORC_OK;
}

/* SuffixAlgo.getPrevRange, F/findex.scala:33-35, over the sampled occ, for k (sp, ep, c) triples: the same two values
 * orc_get_prev_range writes (a = cf(c) + occ(c, sp - 1), b = cf(c) + occ(c, ep - 1)); an empty range is a >= b.  One call is
 * one level of a regex frontier on an index the inverted lists cannot describe. */
int orc_sampled_prev_range_batch(const orc_sampled *s, const uint64_t *sp, const uint64_t *ep, const uint8_t *c,
                                 uint64_t *sp1, uint64_t *ep1, uint64_t k, int threads) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 256) num_threads(threads > 0 ? threads : 1)
#endif
  for (int64_t q = 0; q < (int64_t)k; q++) {
    const int ch = c[q];
    sp1[q] = (uint64_t)((int64_t)s->bs[ch] + sampled_occ(s, ch, (int64_t)sp[q] - 1));
    ep1[q] = (uint64_t)((int64_t)s->bs[ch] + sampled_occ(s, ch, (int64_t)ep[q] - 1));
  }
  (void)threads;
  return ORC_OK;
}
