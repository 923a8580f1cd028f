// gswt_api_comm.hip -- sharding and the framebuffer gather of libgswt_hip.so (host only): the shard geometry and its exported
// primitives, the re-assembly of gathered shards (k_unshard, gswt_kernels.hip), and the two gather transports -- an RCCL
// communicator (one process per GPU) or a local group of contexts (one process, peer copies).
#include "gswt_ctx.h"

#include <dlfcn.h>

#include <algorithm>

using namespace gswt;

namespace {

// RCCL through dlopen: a single-GPU host never needs the library, and a process that already holds one (PyTorch-ROCm bundles
// its own librccl.so) gets that copy instead of a second one.
struct Id128 { char b[GSWT_COMM_ID_BYTES]; };
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, /* ncclUniqueId by value: 128 bytes */ Id128, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool tried = false;
};
RcclApi g_rccl;

const char* rccl_load()
{
    if (g_rccl.lib) return nullptr;
    if (g_rccl.tried) return "librccl.so could not be loaded";
    g_rccl.tried = true;
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
        g_rccl.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (g_rccl.lib) break;
    }
    if (!g_rccl.lib) return "librccl.so could not be loaded";
    g_rccl.GetUniqueId = reinterpret_cast<int (*)(void*)>(dlsym(g_rccl.lib, "ncclGetUniqueId"));
    g_rccl.CommInitRank = reinterpret_cast<int (*)(void**, int, Id128, int)>(dlsym(g_rccl.lib, "ncclCommInitRank"));
    g_rccl.AllGather = reinterpret_cast<int (*)(const void*, void*, size_t, int, void*, hipStream_t)>(dlsym(g_rccl.lib, "ncclAllGather"));
    g_rccl.CommDestroy = reinterpret_cast<int (*)(void*)>(dlsym(g_rccl.lib, "ncclCommDestroy"));
    g_rccl.GetErrorString = reinterpret_cast<const char* (*)(int)>(dlsym(g_rccl.lib, "ncclGetErrorString"));
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy) {
        dlclose(g_rccl.lib); g_rccl.lib = nullptr;
        return "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy";
    }
    return nullptr;
}

constexpr int kNcclFloat = 7;      // ncclFloat32 (rccl.h ncclDataType_t)

}  // namespace

void gswt::rccl_comm_destroy(void* comm)
{
    if (g_rccl.CommDestroy) g_rccl.CommDestroy(comm);
}

ShardGeom gswt::shard_geom(const gswt_render_config& cfg, int width, int height)
{
    ShardGeom g;
    g.world = cfg.shard_count <= 1 ? 1 : cfg.shard_count;
    g.cols = g.world > 1 && cfg.shard_mode == GSWT_SHARD_COLUMNS;
    g.rows_padded = gswt_shard_rows_padded(height, g.world);
    g.band_px = cfg.shard_mode == GSWT_SHARD_COLUMNS ? gswt_shard_cols_padded(width, g.world) : 0;
    g.out_rows = g.world > 1 && !g.cols ? g.rows_padded : height;
    g.out_w = g.cols ? g.band_px : width;
    g.px = (size_t)g.out_rows * g.out_w;
    g.bytes = out_image_bytes((int)cfg.out_format, g.out_rows, g.out_w);
    const int tiles_x = (width + kTile - 1) / kTile;
    g.band_tiles = g.cols ? g.band_px / kTile : tiles_x;
    g.col0 = g.cols ? std::min(cfg.shard_index * g.band_tiles, tiles_x) : 0;
    g.col1 = g.cols ? std::min(g.col0 + g.band_tiles, tiles_x) : tiles_x;
    g.out_x0 = g.cols ? cfg.shard_index * g.band_px : 0;
    return g;
}

extern "C" {

int gswt_shard_rows_padded(int height, int shard_count)
try {
    int tiles_y = (height + kTile - 1) / kTile;
    int sc = shard_count <= 1 ? 1 : shard_count;
    return ((tiles_y + sc - 1) / sc) * kTile;
} GSWT_CATCH

int gswt_shard_cols_padded(int width, int shard_count)
try {
    int tiles_x = (width + kTile - 1) / kTile;
    int sc = shard_count <= 1 ? 1 : shard_count;
    return ((tiles_x + sc - 1) / sc) * kTile;
} GSWT_CATCH

int gswt_shard_rows(int height, int shard_index, int shard_count)
try {
    int sc = shard_count <= 1 ? 1 : shard_count;
    if (shard_index < 0 || shard_index >= sc) return 0;
    int rows = 0;
    for (int y = 0; y < height; y++) if (((y / kTile) % sc) == shard_index) rows++;
    return rows;
} GSWT_CATCH

int gswt_unshard(gswt_ctx* c, const float* gathered, int width, int height, int shard_count, float* out_rgba)
try {
    return gswt_unshard_mode(c, gathered, width, height, shard_count, GSWT_SHARD_ROWS, out_rgba);
} GSWT_CATCH

size_t gswt_out_image_bytes(int out_format, int rows, int out_w) { return out_image_bytes(out_format, rows, out_w); }

int gswt_unshard_mode(gswt_ctx* c, const float* gathered, int width, int height, int shard_count, int shard_mode, float* out_rgba)
try {
    return gswt_unshard_format(c, gathered, width, height, shard_count, shard_mode, GSWT_OUT_RGBA32F, out_rgba);
} GSWT_CATCH

int gswt_unshard_format(gswt_ctx* c, const void* gathered, int width, int height, int shard_count, int shard_mode, int out_format, void* out)
try {
    if (!c || !gathered || !out || width <= 0 || height <= 0 || shard_count < 1) return GSWT_ERR_BAD_ARG;
    if (shard_mode != GSWT_SHARD_ROWS && shard_mode != GSWT_SHARD_COLUMNS) return GSWT_ERR_BAD_ARG;
    if (out_image_bytes(out_format, height, width) == 0) return GSWT_ERR_BAD_ARG;      // unknown format, or a video format at an odd size
    hipSetDevice(c->device);
    gswt_render_config cfg = {};
    cfg.shard_count = shard_count; cfg.shard_mode = shard_mode; cfg.out_format = (uint32_t)out_format;
    const ShardGeom g = shard_geom(cfg, width, height);
    launch_unshard(c->stream, gathered, out, width, height, shard_count, g.rows_padded, g.band_px, out_format);
    HIP_TRY(c, hipGetLastError());
    return GSWT_OK;
} GSWT_CATCH

// ---- multi-GPU gather ------------------------------------------------------------------------------------------------
int gswt_comm_unique_id(void* id_out)
try {
    if (!id_out) return GSWT_ERR_BAD_ARG;
    if (rccl_load()) return GSWT_ERR_RCCL;
    return g_rccl.GetUniqueId(id_out) == 0 ? GSWT_OK : GSWT_ERR_RCCL;
} catch (...) { return GSWT_ERR_RCCL; }

int gswt_comm_init(gswt_ctx* c, const void* unique_id, int rank, int world)
try {
    if (!c || !unique_id || world < 1 || rank < 0 || rank >= world) return fail(c, GSWT_ERR_BAD_ARG, "gswt_comm_init: bad rank / world");
    if (c->comm || !c->group.empty()) return fail(c, GSWT_ERR_STATE, "gswt_comm_init: the ctx already has a communicator (gswt_comm_destroy first)");
    if (const char* e = rccl_load()) return fail(c, GSWT_ERR_RCCL, "gswt_comm_init: %s", e);
    hipSetDevice(c->device);
    Id128 id;
    memcpy(id.b, unique_id, GSWT_COMM_ID_BYTES);
    void* comm = nullptr;
    const int rc = g_rccl.CommInitRank(&comm, world, id, rank);
    if (rc != 0) return fail(c, GSWT_ERR_RCCL, "ncclCommInitRank(rank %d of %d): %s", rank, world, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
    c->comm = comm; c->comm_rank = rank; c->comm_world = world;
    return GSWT_OK;
} GSWT_CATCH

int gswt_comm_destroy(gswt_ctx* c)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    hipSetDevice(c->device);
    HIP_TRY(c, collect_pending(c));
    if (c->comm) { g_rccl.CommDestroy(c->comm); c->comm = nullptr; c->comm_world = 0; }
    // a peer-copy group is dissolved as a whole: no member keeps a pointer to a context that may be destroyed next
    const std::vector<gswt_ctx*> members = c->group;
    for (gswt_ctx* m : members)
        if (m && m != c) { hipSetDevice(m->device); collect_pending(m); m->group.clear(); }
    c->group.clear();
    hipSetDevice(c->device);
    return GSWT_OK;
} GSWT_CATCH

int gswt_group_init(gswt_ctx* const* ctxs, int n)
try {
    if (!ctxs || n < 1) return GSWT_ERR_BAD_ARG;
    for (int r = 0; r < n; r++) {
        if (!ctxs[r]) return GSWT_ERR_BAD_ARG;
        if (ctxs[r]->comm || !ctxs[r]->group.empty()) return fail(ctxs[r], GSWT_ERR_STATE, "gswt_group_init: rank %d already has a communicator", r);
    }
    for (int r = 0; r < n; r++) {
        gswt_ctx* c = ctxs[r];
        hipSetDevice(c->device);
        for (int p = 0; p < n; p++)
            if (ctxs[p]->device != c->device) {
                int can = 0;
                HIP_TRY(c, hipDeviceCanAccessPeer(&can, c->device, ctxs[p]->device));
                if (can) { hipError_t e = hipDeviceEnablePeerAccess(ctxs[p]->device, 0); if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_TRY(c, e); (void)hipGetLastError(); }
            }
        if (!c->ev_push) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_push, hipEventDisableTiming));
        if (!c->ev_unshard) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_unshard, hipEventDisableTiming));
        c->group.assign(ctxs, ctxs + n);
        c->group_rank = r;
    }
    return GSWT_OK;
} catch (...) { return GSWT_ERR_HIP; }

int gswt_render_gather(gswt_ctx* c, int ticket, float* frame_out_dev)
try {
    if (!c || ticket < 0 || ticket >= kFrameSlots || !frame_out_dev) return GSWT_ERR_BAD_ARG;
    if (!c->comm) return fail(c, GSWT_ERR_STATE, "gswt_render_gather before gswt_comm_init");
    int rc = gswt_render_fence(c, ticket);               // overflow-safe: the gathered shard is complete
    if (rc != GSWT_OK) return rc;
    FrameSlot& sl = c->slots[ticket];
    const ShardGeom g = shard_geom(sl.args.cfg, sl.args.width, sl.args.height);
    if (g.world != c->comm_world || sl.args.cfg.shard_index != c->comm_rank)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_render_gather: the frame was rendered as shard %d of %d, the communicator is rank %d of %d",
                    sl.args.cfg.shard_index, g.world, c->comm_rank, c->comm_world);
    hipSetDevice(c->device);
    if (g.world == 1) {                                   // nothing to gather: the shard is the frame
        if (reinterpret_cast<float4*>(frame_out_dev) != sl.args.img.d_out)
            HIP_TRY(c, hipMemcpyAsync(frame_out_dev, sl.args.img.d_out, g.bytes, hipMemcpyDeviceToDevice, c->stream));
        return GSWT_OK;
    }
    HIP_TRY(c, c->gather_buf.ensure(((size_t)g.world * g.bytes + 15) / 16));
    // (the shard moves as 4-byte words whatever its format: g.bytes is a multiple of 4)
    const int nrc = g_rccl.AllGather(sl.args.img.d_out, c->gather_buf.p, g.bytes / 4, kNcclFloat, c->comm, c->stream);
    if (nrc != 0) return fail(c, GSWT_ERR_RCCL, "ncclAllGather: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(nrc) : "error");
    launch_unshard(c->stream, c->gather_buf.p, frame_out_dev, sl.args.width, sl.args.height, g.world, g.rows_padded, g.band_px,
                   (int)sl.args.cfg.out_format);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(sl.ev_gather, c->stream));
    sl.gather_recorded = true;
    return GSWT_OK;
} GSWT_CATCH

int gswt_group_render_gather(gswt_ctx* const* ctxs, const int* tickets, float* const* frames_out_dev, int n)
try {
    if (!ctxs || !tickets || !frames_out_dev || n < 1) return GSWT_ERR_BAD_ARG;
    for (int r = 0; r < n; r++)
        if (!ctxs[r] || (int)ctxs[r]->group.size() != n || ctxs[r]->group[r] != ctxs[r] || !frames_out_dev[r] || tickets[r] < 0 || tickets[r] >= kFrameSlots)
            return GSWT_ERR_BAD_ARG;
    // 1. every rank's frame is complete (overflow-safe fence) and the ctx streams are ordered behind them
    for (int r = 0; r < n; r++) { int rc = gswt_render_fence(ctxs[r], tickets[r]); if (rc != GSWT_OK) return rc; }
    const FrameArgs& a0 = ctxs[0]->slots[tickets[0]].args;
    const ShardGeom g0 = shard_geom(a0.cfg, a0.width, a0.height);
    const int fmt0 = (int)a0.cfg.out_format;
    for (int r = 0; r < n; r++) {
        gswt_ctx* c = ctxs[r];
        const FrameSlot& sl = c->slots[tickets[r]];
        const ShardGeom g = shard_geom(sl.args.cfg, sl.args.width, sl.args.height);
        if (g.world != n || sl.args.cfg.shard_index != r || sl.args.cfg.shard_mode != a0.cfg.shard_mode || g.px != g0.px || sl.args.width != a0.width)
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_group_render_gather: rank %d rendered shard %d of %d", r, sl.args.cfg.shard_index, g.world);
        if ((int)sl.args.cfg.out_format != fmt0)
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_group_render_gather: rank %d rendered out_format %d, rank 0 out_format %d", r, (int)sl.args.cfg.out_format, fmt0);
    }
    for (int r = 0; r < n; r++) {
        gswt_ctx* c = ctxs[r];
        hipSetDevice(c->device);
        HIP_TRY(c, c->gather_buf.ensure(((size_t)n * g0.bytes + 15) / 16));
    }
    // 2. push: rank r copies its shard into slot r of every peer's gather buffer (xGMI peer copies; a plain copy on one device).
    // A peer's gather buffer may still be read by the re-assembly of the PREVIOUS gather on the peer's own stream (gathers are
    // issued back to back with frames in flight): the pushing stream first waits for that re-assembly (write-after-read).
    for (int r = 0; r < n; r++) {
        gswt_ctx* c = ctxs[r];
        hipSetDevice(c->device);
        const FrameSlot& sl = c->slots[tickets[r]];
        for (int p = 0; p < n; p++)
            if (p != r && ctxs[p]->unshard_pending) HIP_TRY(c, hipStreamWaitEvent(c->stream, ctxs[p]->ev_unshard, 0));
        for (int p = 0; p < n; p++)
            HIP_TRY(c, hipMemcpyPeerAsync(reinterpret_cast<char*>(ctxs[p]->gather_buf.p) + (size_t)r * g0.bytes, ctxs[p]->device, sl.args.img.d_out, c->device,
                                          g0.bytes, c->stream));
        HIP_TRY(c, hipEventRecord(c->ev_push, c->stream));
    }
    // 3. every rank waits (on the device) for all pushes, then re-assembles the frame
    for (int p = 0; p < n; p++) {
        gswt_ctx* c = ctxs[p];
        hipSetDevice(c->device);
        const FrameSlot& sl = c->slots[tickets[p]];
        for (int r = 0; r < n; r++) HIP_TRY(c, hipStreamWaitEvent(c->stream, ctxs[r]->ev_push, 0));
        if (n == 1) {
            if (reinterpret_cast<float4*>(frames_out_dev[p]) != sl.args.img.d_out)
                HIP_TRY(c, hipMemcpyAsync(frames_out_dev[p], c->gather_buf.p, g0.bytes, hipMemcpyDeviceToDevice, c->stream));
        } else {
            launch_unshard(c->stream, c->gather_buf.p, frames_out_dev[p], sl.args.width, sl.args.height, n, g0.rows_padded, g0.band_px, fmt0);
            HIP_TRY(c, hipGetLastError());
        }
        HIP_TRY(c, hipEventRecord(c->ev_unshard, c->stream));
        c->unshard_pending = true;
        FrameSlot& slw = c->slots[tickets[p]];
        HIP_TRY(c, hipEventRecord(slw.ev_gather, c->stream));
        slw.gather_recorded = true;
    }
    return GSWT_OK;
} catch (...) { return GSWT_ERR_HIP; }

}  // extern "C"
