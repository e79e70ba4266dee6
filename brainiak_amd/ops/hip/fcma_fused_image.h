// Address arithmetic of k_corr_gram_fused's z image in LDS.  The kernel
// and the host-side hook that the layout tests read
// (fcma_fused_image_layout) evaluate these very functions.
//
// One image holds a window of normalized z for the FS_CB = 16 selected
// voxels of a workgroup: voxel c at c * stride, its 64 epoch rows of 64 B
// (32 columns of bf16) at e * 64.  A row is four 16-B chunks; chunk k
// (columns 8k .. 8k+7) sits in slot k ^ fs_img_swz(e).
//
// What the two accesses need on gfx950:
//
//  Stores.  A task's ds_write_b64 is served in four groups of 16
//  contiguous lanes, banks (a/4) mod 32.  A group has q = lane>>4 fixed
//  and lane&15 = the 16 voxels, so its addresses differ by multiples of
//  the stride alone.  The stride is 4096 + 16 B = 1028 dwords = 4 mod 32:
//  the 16 lanes fall on 8 bank positions of 2 dwords each, two lanes on
//  each, a 2-way conflict (8 array cycles).  With a 16-byte-aligned
//  stride and every lane of a group on the same 8-byte half of its chunk
//  that is the floor; any stride whose sixteenth is odd reaches it.  (The
//  4096 + 32 B this image had before put the group on 4 positions: 4-way,
//  16 cycles.)
//
//  Gram reads.  A band's ds_read_b128 (lane -> row band*16 + lane&15,
//  chunk q) is served in four groups of 16 lanes that are NOT contiguous,
//  banks (a/4) mod 64:
//      {0-3, 12-15, 20-27}   {4-11, 16-19, 28-31}
//      {32-35, 44-47, 52-59} {36-43, 48-51, 60-63}
//  so a group holds chunk q of the rows with h = (e>>2)&3 in {0, 3} and
//  chunk q^1 of the rows with h in {1, 2} (or the other way round).  Four
//  consecutive rows fill one 256-B bank row, so the 16 lanes are
//  conflict-free exactly when the four (q, h) combinations of a group
//  land in four different slots.  fs_img_swz(e) = (4 - h) & 3, the map
//  0, 3, 2, 1, does that: q ^ {0, 1} for h in {0, 3} and
//  (q^1) ^ {3, 2} = q ^ {2, 3} for h in {1, 2}.  (The plain XOR with h,
//  right for contiguous groups, gave q ^ {0, 3} twice: 2-way.)
//
// The swizzle term depends on e only through (e>>2)&3.  In the writer
// e = (wave + 8*si)*P + p with 8*si*P a multiple of 16 and p < P <= 4,
// P | 4: (e>>2)&3 = ((wave*P)>>2)&3 whatever si and p are, so a lane's
// slot is fixed per sub-tile and the store address is one base per
// sub-tile plus an immediate (fs_img_store_base + fs_img_store_step).

#pragma once

#if defined(__HIPCC__)
#define FS_IMG_HD __host__ __device__ __forceinline__
#else
#define FS_IMG_HD inline
#endif

#define FS_IMG_CB 16        // voxels per image
#define FS_IMG_E 64         // epoch rows per voxel
#define FS_IMG_ROWB 64      // bytes per row: 32 columns of bf16
#define FS_IMG_NW 8         // waves per workgroup

// bytes from one voxel's rows to the next
FS_IMG_HD constexpr unsigned fs_img_stride() {
    return FS_IMG_E * FS_IMG_ROWB + 16;
}

// bytes of one image (the kernel keeps two, back to back)
FS_IMG_HD constexpr unsigned fs_img_bytes() {
    return FS_IMG_CB * fs_img_stride();
}

// slot of chunk k in row e is k ^ fs_img_swz(e)
FS_IMG_HD constexpr unsigned fs_img_swz(unsigned e) {
    return (4u - ((e >> 2) & 3u)) & 3u;
}

// Writer, per lane and sub-tile st: the 8 bytes of columns
// st*16 + 4q .. +3 (q = lane>>4) of voxel lane&15, for the wave's first
// subject and epoch p = 0
FS_IMG_HD constexpr unsigned fs_img_store_base(int P, int wave, int st,
                                              int lane) {
    const unsigned l16 = lane & 15, q = lane >> 4;
    const unsigned e0 = (unsigned)(wave * P);
    return l16 * fs_img_stride() + e0 * FS_IMG_ROWB
        + (((st * 2 + (q >> 1)) ^ fs_img_swz(e0)) << 4) + (q & 1) * 8;
}

// ... and the immediate that takes it to subject wave + 8*si, epoch p
FS_IMG_HD constexpr unsigned fs_img_store_step(int P, int si, int p) {
    return (unsigned)(si * FS_IMG_NW * P + p) * FS_IMG_ROWB;
}

FS_IMG_HD constexpr unsigned fs_img_store_offset(int P, int wave, int si,
                                                int st, int p, int lane) {
    return fs_img_store_base(P, wave, st, lane)
        + fs_img_store_step(P, si, p);
}

// Gram reader: the 16 bytes of columns 8q .. 8q+7 (q = lane>>4) of row
// band*16 + lane&15 of a voxel
FS_IMG_HD constexpr unsigned fs_img_read_offset(int voxel, int band,
                                               int lane) {
    const unsigned e = band * 16 + (lane & 15), q = lane >> 4;
    return voxel * fs_img_stride() + e * FS_IMG_ROWB
        + ((q ^ fs_img_swz(e)) << 4);
}
