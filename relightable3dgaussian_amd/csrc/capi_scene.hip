// C ABI of the scene assembly (include/r3dg_hip.h): PLY records <-> parameter groups, objects into a composite, the 8-bit
// quantisation of a frame, and its counterpart on the input side, the unpacking of a stored 8-bit ground-truth view.  Set-up,
// input and output paths, outside the per-stage timing of a training iteration or a relight frame.
#include "capi_internal.hpp"

using namespace r3dg;

namespace {

// a host table of R3DG_SCENE_GROUPS device pointers -> SceneGroups; `required`: how many leading entries must be non-NULL, and
// the remaining ones must then be all set or all NULL
bool read_groups(void** table, int required, bool rest_optional, SceneGroups& out)
{
    if (!table) return false;
    int rest = 0;
    for (int g = 0; g < R3DG_SCENE_GROUPS; g++) {
        out.p[g] = (float*)table[g];
        if (g < required && !table[g]) return false;
        if (g >= required && table[g]) rest++;
    }
    if (rest_optional) return rest == 0 || rest == R3DG_SCENE_GROUPS - required;
    return rest == R3DG_SCENE_GROUPS - required;
}

int check_placement(const char* who, int P, long long row_offset, const float* placement, int flags)
{
    if (P < 0 || row_offset < 0) return invalid(std::string(who) + ": bad row count or offset");
    if (flags & ~(R3DG_SCENE_ZERO_INCIDENTS | R3DG_SCENE_ROTATE_SH)) return invalid(std::string(who) + ": unknown flag");
    if ((flags & R3DG_SCENE_ROTATE_SH) && !placement) return invalid(std::string(who) + ": rotate_sh needs a placement");
    return R3DG_OK;
}

}  // namespace

extern "C" {

int r3dg_scene_place_records(void* stream_, int P, int A, const float* records, const int32_t* column_map,
                             const float* placement, int flags, long long row_offset, void** dst_groups)
{
    if (int e = check_placement("scene_place_records", P, row_offset, placement, flags)) return e;
    if (A < R3DG_SCENE_STAGE1_COLUMNS || A > R3DG_SCENE_MAX_COLUMNS) return invalid("scene_place_records: bad column count");
    if (P == 0) return R3DG_OK;
    SceneGroups dst;
    if (!records || !column_map || !read_groups(dst_groups, R3DG_SCENE_GROUPS, false, dst))
        return invalid("scene_place_records: null buffer");
    if ((size_t)records & 3) return invalid("scene_place_records: records must be 4-byte aligned");
    return guarded([&]() -> int {
        launch_scene_place_records((hipStream_t)stream_, P, A, records, column_map, placement, flags, row_offset, dst);
        return R3DG_OK;
    });
}

int r3dg_scene_place_groups(void* stream_, int P, void** src_groups, const float* placement, int flags, long long row_offset,
                            void** dst_groups)
{
    if (int e = check_placement("scene_place_groups", P, row_offset, placement, flags)) return e;
    if (P == 0) return R3DG_OK;
    SceneGroups src, dst;
    if (!read_groups(src_groups, 7, true, src) || !read_groups(dst_groups, R3DG_SCENE_GROUPS, false, dst))
        return invalid("scene_place_groups: null buffer (the six PBR source groups are all present or all absent)");
    return guarded([&]() -> int {
        launch_scene_place_groups((hipStream_t)stream_, P, src, placement, flags, row_offset, dst);
        return R3DG_OK;
    });
}

int r3dg_scene_pack_records(void* stream_, int P, int columns, void** src_groups, float* records)
{
    if (P < 0) return invalid("scene_pack_records: bad P");
    if (columns != R3DG_SCENE_STAGE1_COLUMNS && columns != R3DG_SCENE_COLUMNS)
        return invalid("scene_pack_records: a record holds 62 or 130 columns");
    if (P == 0) return R3DG_OK;
    SceneGroups src;
    if (!records || !read_groups(src_groups, columns == R3DG_SCENE_COLUMNS ? R3DG_SCENE_GROUPS : 7, true, src))
        return invalid("scene_pack_records: null buffer");
    return guarded([&]() -> int {
        launch_scene_pack_records((hipStream_t)stream_, P, columns, src, records);
        return R3DG_OK;
    });
}

int r3dg_relight_quantize(void* stream_, int width, int height, int channels, const float* image, uint8_t* bytes)
{
    if (width < 0 || height < 0 || channels < 1 || channels > 4) return invalid("relight_quantize: bad shape");
    if ((long long)width * height == 0) return R3DG_OK;
    if ((long long)width * height >= (1ll << 31)) return invalid("relight_quantize: image too large");
    if (!image || !bytes) return invalid("relight_quantize: null buffer");
    return guarded([&]() -> int {
        launch_relight_quantize((hipStream_t)stream_, width, height, channels, image, bytes);
        return R3DG_OK;
    });
}

int r3dg_training_sheet(void* stream_, int width, int height, int layout, const float* render, const float* gt,
                        const float* opacity, const int32_t* n_contrib, const float* feature, const float* pseudo_normal,
                        const float* background, const float* env, int env_rows, int out_width, int out_height, uint8_t* bytes)
{
    if (layout != 0 && layout != 1) return invalid("training_sheet: layout is 0 (stage 1, S = 5) or 1 (stage 2, S = 28)");
    if (width < 1 || height < 1 || out_width < 1 || out_height < 1) return invalid("training_sheet: bad shape");
    if ((long long)width * height >= (1ll << 31) || (long long)out_width * out_height >= (1ll << 31) ||
        4ll * ((long long)width + 2) + 2 >= (1ll << 31) || 4ll * ((long long)height + 2) + 2 >= (1ll << 31))
        return invalid("training_sheet: image too large");
    if (!render || !gt || !opacity || !n_contrib || !feature || !pseudo_normal || !bytes)
        return invalid("training_sheet: null buffer");
    if (layout == 1 && (!background || !env || env_rows < 1 || env_rows >= (1 << 14)))
        return invalid("training_sheet: layout 1 needs the background and the environment texture [R,2R,3], 1 <= R < 16384");
    if ((size_t)bytes & 3) return invalid("training_sheet: the sheet must be 4-byte aligned");
    return guarded([&]() -> int {
        launch_training_sheet((hipStream_t)stream_, width, height, layout, render, gt, opacity, n_contrib, feature, pseudo_normal,
                              background, env, env_rows, out_width, out_height, bytes);
        return R3DG_OK;
    });
}

static const char* png_shape_error(int width, int height, int channels)
{
    if (channels < 1 || channels > 4) return "png: 1..4 channels";
    if (width < 1 || height < 1) return "png: bad shape";
    if ((long long)width * channels + 1 > 65535) return "png: a filtered row (width * channels + 1 bytes) must fit 65535 bytes";
    if ((long long)width * height >= (1ll << 31)) return "png: image too large";
    return nullptr;
}

long long r3dg_png_zlib_bound(int width, int height, int channels)
{
    if (const char* e = png_shape_error(width, height, channels)) return invalid(e);
    return png_zlib_bound(width, height, channels);
}

long long r3dg_png_scratch_bytes(int width, int height, int channels)
{
    if (const char* e = png_shape_error(width, height, channels)) return invalid(e);
    return png_scratch_bytes(width, height, channels);
}

int r3dg_png_encode(void* stream_, int width, int height, int channels, const uint8_t* bytes, const uint32_t* code_table,
                    const uint8_t* block_header, int header_bits, uint8_t* scratch, long long scratch_bytes, uint8_t* zlib,
                    long long zlib_capacity, int32_t* zlib_bytes)
{
    if (const char* e = png_shape_error(width, height, channels)) return invalid(e);
    if (header_bits < 17 || header_bits > 2048) return invalid("png_encode: a block header has 17..2048 bits");
    if (!bytes || !code_table || !block_header || !scratch || !zlib || !zlib_bytes) return invalid("png_encode: null buffer");
    const long long bound = png_zlib_bound(width, height, channels);
    if (bound >= (1ll << 31)) return invalid("png_encode: a stream bound of 2^31 bytes and more");
    if (zlib_capacity < bound) return invalid("png_encode: the stream buffer is smaller than r3dg_png_zlib_bound");
    if (scratch_bytes < png_scratch_bytes(width, height, channels))
        return invalid("png_encode: the scratch is smaller than r3dg_png_scratch_bytes");
    if (((size_t)scratch & 15) || ((size_t)code_table & 3) || ((size_t)zlib_bytes & 3))
        return invalid("png_encode: the scratch must be 16-byte aligned, the code table and the length word 4-byte aligned");
    return guarded([&]() -> int {
        launch_png_encode((hipStream_t)stream_, width, height, channels, bytes, code_table, block_header, header_bits, scratch, zlib,
                          zlib_bytes);
        return R3DG_OK;
    });
}

int r3dg_view_unpack(void* stream_, int width, int height, int channels, const uint8_t* pixels, const float* background,
                     float* image, float* mask)
{
    if (width < 0 || height < 0 || (channels != 3 && channels != 4)) return invalid("view_unpack: bad shape (3 or 4 channels)");
    if ((long long)width * height == 0) return R3DG_OK;
    if ((long long)width * height >= (1ll << 31)) return invalid("view_unpack: image too large");
    if (!pixels || !background || !image) return invalid("view_unpack: null buffer");
    return guarded([&]() -> int {
        launch_view_unpack((hipStream_t)stream_, width, height, channels, pixels, background, image, mask);
        return R3DG_OK;
    });
}

int r3dg_view_unpack_masked(void* stream_, int width, int height, const uint8_t* pixels, const uint8_t* mask_bytes, float* image,
                            float* mask)
{
    if (width < 0 || height < 0) return invalid("view_unpack_masked: bad shape");
    if ((long long)width * height == 0) return R3DG_OK;
    if ((long long)width * height >= (1ll << 31)) return invalid("view_unpack_masked: image too large");
    if (!pixels || !mask_bytes || !image) return invalid("view_unpack_masked: null buffer");
    return guarded([&]() -> int {
        launch_view_unpack_masked((hipStream_t)stream_, width, height, pixels, mask_bytes, image, mask);
        return R3DG_OK;
    });
}

int r3dg_view_resize(void* stream_, int width, int height, int channels, const uint8_t* pixels, const uint8_t* mask_bytes,
                     const float* background, int out_width, int out_height, float* image, float* mask)
{
    if (width < 1 || height < 1 || (channels != 3 && channels != 4)) return invalid("view_resize: bad shape (3 or 4 channels)");
    if (out_width < 1 || out_height < 1 || out_width > width || out_height > height)
        return invalid("view_resize: the target is 1 x 1 at least and no larger than the source (no upscaling)");
    if ((long long)out_width * R3DG_VIEW_RESIZE_MAX_SCALE < width || (long long)out_height * R3DG_VIEW_RESIZE_MAX_SCALE < height)
        return invalid("view_resize: a scale above 16");
    if ((long long)width * height >= (1ll << 31)) return invalid("view_resize: image too large");
    if (!pixels || !image || (channels == 4 && !background)) return invalid("view_resize: null buffer");
    if (channels == 4 && mask_bytes) return invalid("view_resize: an RGBA view has its mask in the alpha channel");
    if (((size_t)pixels & 15) || ((size_t)mask_bytes & 15)) return invalid("view_resize: the byte arrays must be 16-byte aligned");
    return guarded([&]() -> int {
        launch_view_resize((hipStream_t)stream_, width, height, channels, pixels, mask_bytes, background, out_width, out_height,
                           image, mask);
        return R3DG_OK;
    });
}

int r3dg_exr_unpack_chunks(void* stream_, int width, int height, int file_channels, int bytes_per_sample, int chunks,
                           int max_chunk_rows, const uint8_t* inflated, long long inflated_bytes, const int32_t* chunk_table,
                           int kept, const int32_t* kept_channels, uint32_t* tile_sums, long long tile_sums_count, void* planes)
{
    if (width < 1 || height < 1 || file_channels < 1 || chunks < 0 || max_chunk_rows < 1 || inflated_bytes < 0)
        return invalid("exr_unpack_chunks: bad shape");
    if (bytes_per_sample != 2 && bytes_per_sample != 4) return invalid("exr_unpack_chunks: samples are 2 (half) or 4 (float) bytes");
    if (kept < 1 || kept > R3DG_EXR_MAX_KEPT) return invalid("exr_unpack_chunks: 1 to 8 kept channels");
    if (chunks > 65535) return invalid("exr_unpack_chunks: more than 65535 chunks");
    if ((long long)width * height >= (1ll << 31)) return invalid("exr_unpack_chunks: image too large");
    if ((long long)max_chunk_rows * width * file_channels * bytes_per_sample >= (1ll << 31) ||
        inflated_bytes >= (1ll << 32))
        return invalid("exr_unpack_chunks: chunk or view too large");
    if (chunks == 0) return R3DG_OK;
    const size_t tiles = exr_tiles_per_chunk(width, file_channels, bytes_per_sample, max_chunk_rows);
    if (tiles > R3DG_EXR_MAX_TILES) return invalid("exr_unpack_chunks: chunk too large");
    if (tile_sums_count < 0 || (size_t)tile_sums_count < (size_t)chunks * 2 * tiles)
        return invalid("exr_unpack_chunks: the tile sum scratch is too small");
    if (!inflated || !chunk_table || !kept_channels || !tile_sums || !planes) return invalid("exr_unpack_chunks: null buffer");
    if (((size_t)inflated & 15) || ((size_t)planes & 3)) return invalid("exr_unpack_chunks: misaligned buffer");
    return guarded([&]() -> int {
        launch_exr_unpack_chunks((hipStream_t)stream_, width, height, file_channels, bytes_per_sample, chunks, max_chunk_rows,
                                 inflated, inflated_bytes, chunk_table, kept, kept_channels, tile_sums, planes);
        return R3DG_OK;
    });
}

int r3dg_view_unpack_hdr(void* stream_, int width, int height, int is_half, const void* view, const uint8_t* mask_bytes,
                         const float* background, float* image, float* mask)
{
    if (width < 0 || height < 0) return invalid("view_unpack_hdr: bad shape");
    if ((long long)width * height == 0) return R3DG_OK;
    if ((long long)width * height >= (1ll << 31)) return invalid("view_unpack_hdr: image too large");
    if (!view || !background || !image) return invalid("view_unpack_hdr: null buffer");
    if ((size_t)view & (is_half ? 1 : 3)) return invalid("view_unpack_hdr: misaligned view");
    return guarded([&]() -> int {
        launch_view_unpack_hdr((hipStream_t)stream_, width, height, is_half, view, mask_bytes, background, image, mask);
        return R3DG_OK;
    });
}

}  // extern "C"
