// Signals and row buckets: CSR upload / download, device ingest, import between contexts,
// synthetic data, and the per-rank row partition with its buckets and solve pieces.
#include <cmath>

#include "ctx.h"

namespace qmfx {

void drop_csr(SideBuf& sb) {
  sb.rowptr.reset();
  sb.col.reset();
  sb.val.reset();
  sb.shard_off = 0;
  sb.sharded = false;
}

void set_default_bounds(SideBuf& sb, int world, int rank) {
  sb.bounds.assign(world + 1, 0);
  const int64_t total = sb.h_rowptr.empty() ? 0 : sb.h_rowptr.back();
  for (int r = 0; r <= world; ++r) {
    if (r == world) {
      sb.bounds[r] = sb.n;
    } else if (r == 0) {
      sb.bounds[r] = 0;
    } else {
      const int64_t target = (int64_t)((__int128)total * r / world);
      sb.bounds[r] = std::lower_bound(sb.h_rowptr.begin(), sb.h_rowptr.end(), target) -
                     sb.h_rowptr.begin();
      if (sb.bounds[r] > sb.n) sb.bounds[r] = sb.n;
    }
  }
  for (int r = 1; r <= world; ++r) sb.bounds[r] = std::max(sb.bounds[r], sb.bounds[r - 1]);
  sb.rbeg = sb.bounds[rank];
  sb.rend = sb.bounds[rank + 1];
}

// nnz-balanced split of rows [b, e) into p contiguous pieces → out[0..p]
static void split_rows(const std::vector<int64_t>& rp, int64_t b, int64_t e, int p, int64_t* out) {
  out[0] = b;
  out[p] = e;
  for (int j = 1; j < p; ++j) {
    const int64_t target = rp[b] + (int64_t)((__int128)(rp[e] - rp[b]) * j / p);
    int64_t r = std::lower_bound(rp.begin() + b, rp.begin() + e + 1, target) - rp.begin();
    out[j] = std::min(std::max(r, out[j - 1]), e);
  }
}

// The all-gather schedule of a half: rank r owns rows [bounds[r], bounds[r+1]) and splits
// them into P nnz-balanced pieces; pb[r·(P+1) + j] .. pb[r·(P+1) + j + 1] is the row range
// rank r broadcasts after solving its piece j (qmfx_wals_half), skipped when empty.
void plan_pieces(const std::vector<int64_t>& rp, const std::vector<int64_t>& bounds, int world,
                 int P, std::vector<int64_t>& pb) {
  pb.assign((size_t)world * (P + 1), 0);
  for (int r = 0; r < world; ++r) split_rows(rp, bounds[r], bounds[r + 1], P, &pb[(size_t)r * (P + 1)]);
}

// a device copy of a host list (at least one element allocated)
template <typename T>
static hipError_t upload(qmfx_ctx* c, DevPtr<T>& d, const std::vector<T>& h) {
  const hipError_t e = dev_alloc(d, std::max<size_t>(h.size(), 1) * sizeof(T));
  return e != hipSuccess ? e : scopy(c, d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

// Splits this rank's rows of `side` into pieces, and each piece into whitened buckets (by
// padded signal count) and the direct bucket (heaviest rows first, for load balance);
// uploads the order list (piece sections back to back) and the per-slot descriptors.
int build_buckets(qmfx_ctx* c, int side) {
  SideBuf& sb = c->s[side];
  sb.buckets_valid = false;
  if (sb.h_rowptr.empty()) return 0;
  if (sb.n > INT32_MAX) return fail("more than 2^31 rows on one side are not supported");
  const int mx = max_whitened_ntn(c);
  const int P = npieces(c);
  plan_pieces(sb.h_rowptr, sb.bounds, c->world, P, sb.pbounds);
  double nnz_w = 0, nnz_d = 0, flops_w = 0;
  const double k = c->k;
  std::vector<int64_t> order;
  order.reserve(sb.rend - sb.rbeg);
  sb.pieces.assign(P, Piece{});
  int64_t nw_total = 0;
  // split-K heavy rows at every k (the multi-wave k > 128 kernel has segment modes too)
  const int64_t hmin = c->heavy_min;
  std::vector<RowDesc> segs, heavy;
  std::vector<int64_t> hseg;
  for (int j = 0; j < P; ++j) {
    Piece& pc = sb.pieces[j];
    pc.rb = sb.pbounds[(size_t)c->rank * (P + 1) + j];
    pc.re = sb.pbounds[(size_t)c->rank * (P + 1) + j + 1];
    pc.ord = (int64_t)order.size();
    std::vector<int64_t> wlist[kMaxNTN];
    std::vector<std::pair<int64_t, int64_t>> direct;
    for (int64_t r = pc.rb; r < pc.re; ++r) {
      const int64_t n = sb.h_rowptr[r + 1] - sb.h_rowptr[r];
      // RowDesc::n is int32 (segments too: seg_len is clamped at create)
      if (n > INT32_MAX) return fail("a row with more than 2^31-1 signals is not supported");
      const int64_t ntn = (std::max<int64_t>(n, 1) + 15) / 16;
      if (ntn <= mx) {
        wlist[ntn - 1].push_back(r);
        nnz_w += (double)n;
        // K (n(n+1)k), n×n Cholesky + solves (n³/3 + 2n²), Zᵀu and Zᵀc (4nk), unwhitening (2k²)
        const double dn = (double)n;
        flops_w += dn * (dn + 1) * k + dn * dn * dn / 3.0 + 2 * dn * dn + 4 * dn * k + 2 * k * k;
      } else {
        direct.emplace_back(n, r);
        nnz_d += (double)n;
      }
    }
    std::stable_sort(direct.begin(), direct.end(),
                     [](const auto& x, const auto& y) { return x.first > y.first; });
    // the heaviest direct rows (n > hmin) lead the direct section; each is cut into
    // segments of seg_len signals
    pc.h0 = (int64_t)heavy.size();
    pc.s0 = (int64_t)segs.size();
    for (const auto& d : direct) {
      if (hmin <= 0 || d.first <= hmin) break;
      const int64_t r = d.second, beg = sb.h_rowptr[r], n = d.first;
      hseg.push_back((int64_t)segs.size());
      heavy.push_back(RowDesc{(int64_t)segs.size(), 0, (int32_t)r});
      for (int64_t o = 0; o < n; o += c->seg_len)
        segs.push_back(RowDesc{beg + o, (int32_t)std::min(c->seg_len, n - o),
                               (int32_t)(heavy.size() - 1)});
    }
    pc.nh = (int64_t)heavy.size() - pc.h0;
    pc.ns = (int64_t)segs.size() - pc.s0;
    for (int i = 0; i < kMaxNTN; ++i) {
      pc.wb[i] = (int64_t)order.size() - pc.ord;
      order.insert(order.end(), wlist[i].begin(), wlist[i].end());
    }
    pc.wb[kMaxNTN] = (int64_t)order.size() - pc.ord;
    nw_total += pc.wb[kMaxNTN];
    for (const auto& d : direct) order.push_back(d.second);
    pc.n_ord = (int64_t)order.size() - pc.ord;
  }
  for (int i = 0; i < kMaxNTN; ++i) sb.wb[i] = 0;
  sb.wb[kMaxNTN] = nw_total;  // whitened rows of this rank (all pieces)
  sb.n_ord = (int64_t)order.size();
  sb.nnz_w = nnz_w;
  sb.nnz_d = nnz_d;
  sb.flops_w = flops_w;
  HIPCHK(upload(c, sb.d_order, order));
  std::vector<RowDesc> desc((size_t)sb.n_ord);
  for (size_t i = 0; i < desc.size(); ++i) {
    const int64_t r = order[i];
    desc[i] = RowDesc{sb.h_rowptr[r], (int32_t)(sb.h_rowptr[r + 1] - sb.h_rowptr[r]), (int32_t)r};
  }
  HIPCHK(upload(c, sb.d_desc, desc));
  hseg.push_back((int64_t)segs.size());
  sb.d_seg.reset();
  sb.d_heavy.reset();
  sb.d_hseg.reset();
  sb.nseg = (int64_t)segs.size();
  sb.nheavy = (int64_t)heavy.size();
  if (sb.nheavy > 0) {
    HIPCHK(upload(c, sb.d_seg, segs));
    HIPCHK(upload(c, sb.d_heavy, heavy));
    HIPCHK(upload(c, sb.d_hseg, hseg));
    if (c->part_cap < sb.nseg) {
      const size_t ntt = (size_t)c->nt * (c->nt + 1) / 2;
      c->partb.reset();  // all three go before the larger ones are allocated
      c->partc.reset();
      HIPCHK(dev_alloc(c->part, (size_t)sb.nseg * ntt * 256 * c->esz));
      HIPCHK(dev_alloc(c->partb, (size_t)sb.nseg * c->kp * c->esz));
      HIPCHK(dev_alloc(c->partc, (size_t)sb.nseg * 2 * sizeof(double)));
      c->part_cap = sb.nseg;
    }
  }
  sb.buckets_valid = true;
  return 0;
}

// Keeps only this rank's signals of a side on the device (col/val of rows rbeg..rend).
int shard_csr(qmfx_ctx* c, SideBuf& sb) {
  if (sb.sharded || !sb.col) return 0;
  const int64_t e0 = sb.h_rowptr[sb.rbeg], e1 = sb.h_rowptr[sb.rend];
  const size_t m = (size_t)std::max<int64_t>(e1 - e0, 1);
  DevPtr<int32_t> col;
  DevPtr<void> val;
  HIPCHK(dev_alloc(col, m * sizeof(int32_t)));
  HIPCHK(dev_alloc(val, m * c->esz));
  if (e1 > e0) {
    HIPCHK(hipMemcpyAsync(col, sb.col + e0, (size_t)(e1 - e0) * sizeof(int32_t),
                          hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(val, sb.val.as<char>() + (size_t)e0 * c->esz, (size_t)(e1 - e0) * c->esz,
                          hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  sb.col = std::move(col);
  sb.val = std::move(val);
  sb.shard_off = e0;
  sb.sharded = true;
  return 0;
}

// after a side's CSR and h_rowptr are in place: this rank's rows and their buckets
static int partition_side(qmfx_ctx* c, int side) {
  set_default_bounds(c->s[side], c->world, c->rank);
  return build_buckets(c, side);
}

}  // namespace qmfx

using namespace qmfx;

extern "C" {

int qmfx_upload_csr(qmfx_ctx* c, int side, const int64_t* rowptr, const int32_t* colidx,
                    const double* values, int64_t nnz) {
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  SideBuf& sb = c->s[side];
  if (sb.n <= 0) return fail("shape not set (qmfx_set_shape)");
  sb.h_ids.clear();
  const int64_t nother = c->s[1 - side].n;
  if (rowptr[0] != 0 || rowptr[sb.n] != nnz) return fail("rowptr inconsistent with nnz");
  for (int64_t r = 0; r < sb.n; ++r)
    if (rowptr[r + 1] < rowptr[r]) return fail("rowptr not monotone");
  for (int64_t e = 0; e < nnz; ++e)
    if (colidx[e] < 0 || colidx[e] >= nother) return fail("column index out of range");
  if (set_dev(c)) return -2;
  drop_csr(sb);
  HIPCHK(dev_alloc(sb.rowptr, (size_t)(sb.n + 1) * sizeof(int64_t)));
  HIPCHK(dev_alloc(sb.col, (size_t)std::max<int64_t>(nnz, 1) * sizeof(int32_t)));
  HIPCHK(dev_alloc(sb.val, (size_t)std::max<int64_t>(nnz, 1) * c->esz));
  HIPCHK(scopy(c, sb.rowptr, rowptr, (size_t)(sb.n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (nnz > 0) {
    HIPCHK(scopy(c, sb.col, colidx, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(copy_in(c, sb.val, values, (size_t)nnz));
  }
  sb.nnz = nnz;
  c->nnz = nnz;
  sb.h_rowptr.assign(rowptr, rowptr + sb.n + 1);
  return partition_side(c, side);
}

int qmfx_group_signals(qmfx_ctx* c, const void* records, int64_t nnz, int64_t* nusers,
                       int64_t* nitems) {
  if (nnz <= 0) return fail("empty dataset");
  if (nnz > 0x7fffffffll) return fail("device ingest takes at most 2^31-1 interactions");
  if (set_dev(c)) return -2;
  IngestOut o;
  {
    DevPtr<void> d_rec;
    HIPCHK(dev_alloc(d_rec, (size_t)nnz * 24));
    hipError_t e = scopy(c, d_rec, records, (size_t)nnz * 24, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = group_records(d_rec, nnz, c->prec, o, c->stream);
    if (e != hipSuccess) return fail(std::string("device ingest: ") + hipGetErrorString(e), -2);
  }
  if (int rc = qmfx_set_shape(c, o.n[0], o.n[1])) return rc;
  for (int side = 0; side < 2; ++side) {
    SideBuf& sb = c->s[side];
    drop_csr(sb);
    sb.rowptr = std::move(o.rowptr[side]);
    sb.col = std::move(o.col[side]);
    sb.val = std::move(o.val[side]);
    sb.nnz = nnz;
    sb.h_ids.resize((size_t)sb.n);
    sb.h_rowptr.resize((size_t)sb.n + 1);
    hipError_t e = scopy(c, sb.h_ids.data(), o.ids[side], (size_t)sb.n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      e = scopy(c, sb.h_rowptr.data(), sb.rowptr, (size_t)(sb.n + 1) * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(std::string("device ingest: ") + hipGetErrorString(e), -2);
    set_default_bounds(sb, c->world, c->rank);
  }
  c->nnz = nnz;
  for (int side = 0; side < 2; ++side)
    if (int rc = build_buckets(c, side)) return rc;
  if (nusers) *nusers = c->s[0].n;
  if (nitems) *nitems = c->s[1].n;
  return 0;
}

int qmfx_import_signals(qmfx_ctx* dst, qmfx_ctx* src) {
  if (!dst || !src || dst == src) return fail("qmfx_import_signals: two distinct contexts needed");
  if (dst->prec != src->prec) return fail("qmfx_import_signals: contexts differ in precision");
  for (int side = 0; side < 2; ++side) {
    const SideBuf& s = src->s[side];
    if (!s.rowptr || !s.col || s.h_rowptr.empty()) return fail("qmfx_import_signals: the source has no CSR");
    if (s.sharded) return fail("qmfx_import_signals: the source CSR is sharded");
  }
  // the destination takes a whole CSR: one already partitioned into ranks would be overwritten
  if (dst->comm || dst->world > 1 || dst->s[0].sharded || dst->s[1].sharded)
    return fail("qmfx_import_signals: the destination already went through qmfx_dist_init");
  // the source's CSR writes (its own stream) complete before the copies on dst's stream
  if (set_dev(src)) return -2;
  HIPCHK(hipStreamSynchronize(src->stream));
  if (int rc = qmfx_set_shape(dst, src->s[0].n, src->s[1].n)) return rc;
  if (set_dev(dst)) return -2;
  for (int side = 0; side < 2; ++side) {
    const SideBuf& s = src->s[side];
    SideBuf& d = dst->s[side];
    drop_csr(d);
    const size_t m = (size_t)std::max<int64_t>(s.nnz, 1);
    HIPCHK(dev_alloc(d.rowptr, (size_t)(s.n + 1) * sizeof(int64_t)));
    HIPCHK(dev_alloc(d.col, m * sizeof(int32_t)));
    HIPCHK(dev_alloc(d.val, m * dst->esz));
    // device to device over xGMI (the same device: a plain copy)
    HIPCHK(hipMemcpyPeerAsync(d.rowptr, dst->device, s.rowptr, src->device,
                              (size_t)(s.n + 1) * sizeof(int64_t), dst->stream));
    if (s.nnz > 0) {
      HIPCHK(hipMemcpyPeerAsync(d.col, dst->device, s.col, src->device,
                                (size_t)s.nnz * sizeof(int32_t), dst->stream));
      HIPCHK(hipMemcpyPeerAsync(d.val, dst->device, s.val, src->device, (size_t)s.nnz * dst->esz,
                                dst->stream));
    }
    d.nnz = s.nnz;
    d.h_rowptr = s.h_rowptr;
    d.h_ids = s.h_ids;
  }
  HIPCHK(hipStreamSynchronize(dst->stream));
  dst->nnz = src->nnz;
  for (int side = 0; side < 2; ++side)
    if (int rc = partition_side(dst, side)) return rc;
  return 0;
}

int qmfx_get_ids(qmfx_ctx* c, int side, int64_t* ids) {
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  const SideBuf& sb = c->s[side];
  if ((int64_t)sb.h_ids.size() != sb.n) return fail("no id table: the CSR was not built by qmfx_group_signals");
  std::copy(sb.h_ids.begin(), sb.h_ids.end(), ids);
  return 0;
}

int qmfx_download_csr(qmfx_ctx* c, int side, int64_t* rowptr, int32_t* colidx, double* values) {
  SideBuf& sb = c->s[side];
  if (!sb.rowptr) return fail("no CSR for this side");
  if (sb.sharded) return fail("the CSR is sharded over ranks (qmfx_dist_init): only this rank's rows are held");
  if (set_dev(c)) return -2;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(scopy(c, rowptr, sb.rowptr, (size_t)(sb.n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (sb.nnz > 0) {
    HIPCHK(scopy(c, colidx, sb.col, (size_t)sb.nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(copy_out(c, values, sb.val, (size_t)sb.nnz));
  }
  return 0;
}

int qmfx_gen_synthetic(qmfx_ctx* c, int64_t nusers, int64_t nitems, int64_t nnz, uint64_t seed,
                       int64_t* nnz_out) {
  return qmfx_gen_synthetic_zipf(c, nusers, nitems, nnz, seed, 0.0, nnz_out);
}

int qmfx_gen_synthetic_zipf(qmfx_ctx* c, int64_t nusers, int64_t nitems, int64_t nnz,
                            uint64_t seed, double zipf_s, int64_t* nnz_out) {
  if (nnz <= 0) return fail("nnz must be positive");
  if (zipf_s < 0.0 || !std::isfinite(zipf_s)) return fail("zipf exponent must be >= 0");
  if (int rc = qmfx_set_shape(c, nusers, nitems)) return rc;
  const uint64_t space = (uint64_t)nusers * (uint64_t)nitems;
  if (zipf_s == 0.0 && (uint64_t)nnz > space / 2) return fail("nnz too large for the shape");
  if (nnz > 0x7fffffffll) return fail("at most 2^31-1 draws");
  int end_bit = 64 - __builtin_clzll(space);
  DevPtr<uint64_t> keys, scratch;
  HIPCHK(dev_alloc(keys, (size_t)nnz * 8));
  HIPCHK(dev_alloc(scratch, (size_t)nnz * 8));
  if (zipf_s == 0.0)
    HIPCHK(launch_synth_keys(keys, nnz, space, seed, c->stream));
  else
    HIPCHK(launch_synth_keys_zipf(keys, nnz, (uint64_t)nusers, (uint64_t)nitems, zipf_s, seed,
                                  c->stream));
  int64_t m = 0;
  HIPCHK(sort_unique_keys(keys, scratch, nnz, &m, end_bit, c->stream));
  for (int side = 0; side < 2; ++side) {
    SideBuf& sb = c->s[side];
    drop_csr(sb);
    HIPCHK(dev_alloc(sb.rowptr, (size_t)(sb.n + 1) * sizeof(int64_t)));
    HIPCHK(dev_alloc(sb.col, (size_t)m * sizeof(int32_t)));
    HIPCHK(dev_alloc(sb.val, (size_t)m * c->esz));
    sb.nnz = m;
  }
  // users: keys are u·nitems + i, sorted
  HIPCHK(build_csr_from_sorted_keys(keys, m, nusers, (uint64_t)nitems, c->s[0].rowptr,
                                    c->s[0].col, c->stream));
  HIPCHK(launch_synth_values_any(keys, m, (uint64_t)nitems, (uint64_t)nitems, 1, seed * 31 + 7,
                                 c->s[0].val, c->prec, c->stream));
  // items: transposed keys i·nusers + u, sorted
  HIPCHK(launch_transpose_keys(keys, m, (uint64_t)nitems, (uint64_t)nusers, scratch, c->stream));
  HIPCHK(sort_keys(scratch, keys, m, end_bit, c->stream));
  HIPCHK(build_csr_from_sorted_keys(scratch, m, nitems, (uint64_t)nusers, c->s[1].rowptr,
                                    c->s[1].col, c->stream));
  HIPCHK(launch_synth_values_any(scratch, m, (uint64_t)nusers, (uint64_t)nitems, 0, seed * 31 + 7,
                                 c->s[1].val, c->prec, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  keys.reset();
  scratch.reset();
  for (int side = 0; side < 2; ++side) {
    SideBuf& sb = c->s[side];
    sb.h_rowptr.resize(sb.n + 1);
    HIPCHK(scopy(c, sb.h_rowptr.data(), sb.rowptr, (size_t)(sb.n + 1) * 8, hipMemcpyDeviceToHost));
    if (int rc = partition_side(c, side)) return rc;
  }
  c->nnz = m;
  if (nnz_out) *nnz_out = m;
  return 0;
}

}  // extern "C"
