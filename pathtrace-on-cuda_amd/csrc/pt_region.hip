// pt_region.hip — a pixel window or any list of tiles without the full frame (include/pt_api.h: pt_render_tile_list and friends).
//
// A tile is the 8x8 tile of the tile split, numbered row-major over the FULL frame.  The render of a list differs from a rank's render
// in one kernel only (pt_wavefront.hip: wf_init_list takes a stream's tile from the list); this file holds what comes after it — the
// scatter of a list-major tile buffer into a window of the frame — and the host helpers that turn a window into a list.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>

#include "pt_scene.h"

namespace ptd {

// list-major tiles -> the window [x0, x1) x [y0, y1) of the frame, row-major.  One thread per pixel of the listed tiles: the 64 lanes
// of a wave read the 768 contiguous bytes of one tile and write eight 96-byte row pieces.  Pixels of a tile outside the frame or the
// window are dropped; pixels of the window that no listed tile covers are not touched.
__global__ __launch_bounds__(256)
void untile_list(const float* __restrict__ tiles, const int32_t* __restrict__ tileList, long long nPixels, int tiles_x, int W, int H,
                 int x0, int y0, int x1, int y1, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nPixels) return;
    const int tile = tileList[i >> 6], lane = (int)(i & 63);
    const int px = (tile % tiles_x) * kTile + (lane & 7), py = (tile / tiles_x) * kTile + (lane >> 3);
    if (px >= W || py >= H || px < x0 || px >= x1 || py < y0 || py >= y1) return;
    const float r = tiles[3 * i + 0], g = tiles[3 * i + 1], b = tiles[3 * i + 2];
    float* o = out + ((long long)(py - y0) * (x1 - x0) + (px - x0)) * 3;
    o[0] = r; o[1] = g; o[2] = b;
}

}  // namespace ptd

int pt_window_args(const char* who, const PtCamera* cam, int32_t x0, int32_t y0, int32_t x1, int32_t y1)
{
    if (!cam) { pt_set_error("%s: NULL camera", who); return PT_ERR_INVALID; }
    if (cam->W < 2 || cam->H < 2) { pt_set_error("%s: frame %dx%d too small", who, cam->W, cam->H); return PT_ERR_INVALID; }
    if (x0 < 0 || y0 < 0 || x1 > cam->W || y1 > cam->H || x0 >= x1 || y0 >= y1) {
        pt_set_error("%s: window [%d, %d) x [%d, %d) is empty or not inside the %dx%d frame", who, x0, x1, y0, y1, cam->W, cam->H);
        return PT_ERR_INVALID;
    }
    return PT_OK;
}

extern "C" {

int32_t pt_tiles_of_window(const PtCamera* cam, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t* h_tiles, int32_t cap)
{
    const int rc = pt_window_args("pt_tiles_of_window", cam, x0, y0, x1, y1);
    if (rc) return rc;
    if (cap < 0 || (cap > 0 && !h_tiles)) { pt_set_error("pt_tiles_of_window: cap=%d with%s a buffer", cap, h_tiles ? "" : "out"); return PT_ERR_INVALID; }
    const int tiles_x = ptd::tile_grid(cam->W, cam->H).tiles_x;
    const int tx0 = x0 / ptd::kTile, tx1 = (x1 - 1) / ptd::kTile, ty0 = y0 / ptd::kTile, ty1 = (y1 - 1) / ptd::kTile;
    int32_t n = 0;
    for (int ty = ty0; ty <= ty1; ty++)
        for (int tx = tx0; tx <= tx1; tx++, n++)
            if (n < cap) h_tiles[n] = ty * tiles_x + tx;
    return n;
}

int pt_untile_list(const float* d_tiles, const int32_t* h_tiles, int32_t n_tiles, const PtCamera* cam,
                   int32_t x0, int32_t y0, int32_t x1, int32_t y1, float* d_out, void* hip_stream)
{
    if (!d_tiles || !h_tiles || !d_out) { pt_set_error("pt_untile_list: NULL argument"); return PT_ERR_INVALID; }
    const int rc = pt_window_args("pt_untile_list", cam, x0, y0, x1, y1);
    if (rc) return rc;
    const ptd::TileGrid g = ptd::tile_grid(cam->W, cam->H);
    const int tiles_x = g.tiles_x, n_total = g.total;
    if (n_tiles < 1 || n_tiles > n_total) { pt_set_error("pt_untile_list: n_tiles=%d, the frame has %d tiles", n_tiles, n_total); return PT_ERR_INVALID; }
    for (int32_t i = 0; i < n_tiles; i++)      // an entry outside the frame would be a read or write out of bounds; a tile listed twice is only written twice
        if (h_tiles[i] < 0 || h_tiles[i] >= n_total) { pt_set_error("pt_untile_list: entry %d is tile %d, the frame has tiles 0 .. %d", i, h_tiles[i], n_total - 1); return PT_ERR_INVALID; }
    hipStream_t stream = (hipStream_t)hip_stream;
    // the list lives for this call only: allocated, filled and released in stream order
    int32_t* d_list = nullptr;
    HIPCHK(hipMallocAsync((void**)&d_list, (size_t)n_tiles * 4, stream));
    auto body = [&]() -> int {
        HIPCHK(hipMemcpyAsync(d_list, h_tiles, (size_t)n_tiles * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));      // h_tiles is the caller's (pageable) memory: it has been read when the call returns
        const long long nPixels = (long long)n_tiles * ptd::kTilePixels;
        hipLaunchKernelGGL(ptd::untile_list, dim3((unsigned)((nPixels + 255) / 256)), dim3(256), 0, stream,
                           d_tiles, d_list, nPixels, tiles_x, cam->W, cam->H, x0, y0, x1, y1, d_out);
        HIPCHK(hipGetLastError());
        return PT_OK;
    };
    const int r = body();
    const hipError_t fe = hipFreeAsync(d_list, stream);
    if (r) return r;
    HIPCHK(fe);
    return PT_OK;
}

int pt_render_window(PtScene* s, const PtCamera* cam, const PtParams* prm, int32_t x0, int32_t y0, int32_t x1, int32_t y1, float* h_rgb)
{
    if (!s || !prm || !h_rgb) { pt_set_error("pt_render_window: NULL argument"); return PT_ERR_INVALID; }
    const int32_t n = pt_tiles_of_window(cam, x0, y0, x1, y1, nullptr, 0);
    if (n < 0) return n;
    std::vector<int32_t> list((size_t)n);
    (void)pt_tiles_of_window(cam, x0, y0, x1, y1, list.data(), n);
    PtParams p = *prm; p.rank = 0; p.world = 1;
    const int64_t wb = pt_tile_list_work_bytes(cam, &p, n);
    if (wb < 0) return PT_ERR_INVALID;
    const size_t winBytes = (size_t)(x1 - x0) * (size_t)(y1 - y0) * 12;
    HIPCHK(hipSetDevice(s->device));
    DevBuf d_tiles, d_work, d_win;
    HIPCHK(d_tiles.alloc((size_t)pt_tile_list_floats(n) * 4));
    HIPCHK(d_work.alloc((size_t)wb));
    HIPCHK(d_win.alloc(winBytes));
    int rc = pt_render_tile_list(s, cam, &p, list.data(), n, d_tiles.as<float>(), d_work.as<>(), nullptr);
    if (!rc) rc = pt_untile_list(d_tiles.as<float>(), list.data(), n, cam, x0, y0, x1, y1, d_win.as<float>(), nullptr);      // the list covers every pixel of the window
    if (!rc) HIPCHK(hipMemcpy(h_rgb, d_win.as<>(), winBytes, hipMemcpyDeviceToHost));
    return rc;
}

}  // extern "C"
