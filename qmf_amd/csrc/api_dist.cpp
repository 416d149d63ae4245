// Multi-GPU: RCCL communicators and the per-rank row partition (the half's collectives are
// in api_wals.cpp).
#include <cstring>

#include "ctx.h"

using namespace qmfx;

// This rank's row ranges of both sides, the row buckets, and (world > 1) the CSR shard.
static int dist_partition(qmfx_ctx* c) {
  const int rank = c->rank, world = c->world;
  for (int side = 0; side < 2; ++side) {
    SideBuf& sb = c->s[side];
    if (sb.h_rowptr.empty()) continue;
    if (sb.sharded) return fail("qmfx_dist_init: the CSR is already sharded (re-upload it first)");
    set_default_bounds(sb, world, rank);
    if (int rc = build_buckets(c, side)) return rc;
    if (world > 1)
      if (int rc = shard_csr(c, sb)) return rc;
  }
  return 0;
}

extern "C" {

int qmfx_rccl_unique_id(uint8_t* id128) {
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  static_assert(sizeof(id) == 128, "ncclUniqueId size");
  std::memcpy(id128, &id, 128);
  return 0;
}

int qmfx_dist_init(qmfx_ctx* c, int rank, int world, const uint8_t* id128) {
  if (world < 1 || rank < 0 || rank >= world) return fail("bad rank/world");
  if (set_dev(c)) return -2;
  c->rank = rank;
  c->world = world;
  // world = 1 with an id: a one-rank communicator, so a single GPU runs the RCCL calls of
  // the half (the self-broadcasts and the loss all-reduce) — the tests' loopback check
  if (id128) {
    ncclUniqueId id;
    std::memcpy(&id, id128, 128);
    NCCLCHK(ncclCommInitRank(&c->comm, world, id, rank));
    if (!c->comm_stream) HIPCHK(make_stream(c->comm_stream));
  }
  return dist_partition(c);
}

int qmfx_dist_init_all(qmfx_ctx* const* ctxs, int n) {
  if (n < 1 || !ctxs) return fail("qmfx_dist_init_all: no contexts");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  std::vector<int> devs((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i]) return fail("qmfx_dist_init_all: null context");
    if (ctxs[i]->comm) return fail("qmfx_dist_init_all: context already has a communicator");
    devs[(size_t)i] = ctxs[i]->device;
    for (int j = 0; j < i; ++j)
      if (devs[(size_t)j] == devs[(size_t)i])
        return fail("qmfx_dist_init_all: two contexts on device " + std::to_string(devs[(size_t)i]) +
                    " (one GPU per rank)");
    if (devs[(size_t)i] < 0 || devs[(size_t)i] >= ndev)
      return fail("qmfx_dist_init_all: " + std::to_string(n) + " ranks need device " +
                  std::to_string(devs[(size_t)i]) + " but only " + std::to_string(ndev) +
                  " GPU(s) are visible");
  }
  std::vector<ncclComm_t> comms((size_t)n);
  NCCLCHK(ncclCommInitAll(comms.data(), n, devs.data()));
  for (int i = 0; i < n; ++i) {
    qmfx_ctx* c = ctxs[i];
    if (set_dev(c)) return -2;
    c->comm = comms[(size_t)i];
    c->rank = i;
    c->world = n;
    if (!c->comm_stream) HIPCHK(make_stream(c->comm_stream));
    if (int rc = dist_partition(c)) return rc;
  }
  return 0;
}

int qmfx_dist_plan(const int64_t* rowptr, int64_t nrows, int world, int npieces,
                   int64_t* pbounds) {
  if (world < 1) return fail("bad world size");
  if (npieces < 1 || npieces > QMFX_MAX_PIECES) return fail("npieces out of range");
  SideBuf sb;
  sb.n = nrows;
  sb.h_rowptr.assign(rowptr, rowptr + nrows + 1);
  set_default_bounds(sb, world, 0);
  std::vector<int64_t> pb;
  plan_pieces(sb.h_rowptr, sb.bounds, world, npieces, pb);
  std::copy(pb.begin(), pb.end(), pbounds);
  return 0;
}

int qmfx_partition_rows(const int64_t* rowptr, int64_t nrows, int world, int rank,
                        int64_t* begin, int64_t* end) {
  if (world < 1 || rank < 0 || rank >= world) return fail("bad rank/world");
  SideBuf sb;
  sb.n = nrows;
  sb.h_rowptr.assign(rowptr, rowptr + nrows + 1);
  set_default_bounds(sb, world, rank);
  *begin = sb.rbeg;
  *end = sb.rend;
  return 0;
}

}  // extern "C"
