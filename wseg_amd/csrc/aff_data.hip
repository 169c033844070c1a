// aff_data.hip — the label side of AffinityNet training data (voc12/data.py:220-261 under the transforms of aff_train.py:39-60).
//
// The reference concatenates two dense float32 [21][H][W] CRF score stacks with the image, crops the 45 channels into a crop x crop
// float32 container, flips it, block-means 42 channels 8x8 and takes two arg-maxes — per image, on the host.  Almost all of those planes are
// zero (background and the image's few classes carry scores), so the host ships only the planes that hold a value and this kernel rebuilds
// the label map of the dense rule from them: one launch for the batch (blockIdx.y = sample), one byte per 8x8 cell.
//
//   lane = 8 * cell + window row: 8 lanes per output cell, each sums the 8 floats of its window row (left to right), three xor exchanges
//   add the 8 rows; a wave covers 8 neighbouring cells, so per plane it reads eight runs of 64 floats.  img_left and W are arbitrary: the
//   loads are 4-byte loads, nothing assumes a wider alignment.  The summation order is fixed, there are no atomics and no LDS: the bytes are
//   the same from run to run.  Outside the pasted rectangle the container is 0; the mean always divides by 64.  The flip mirrors cell columns
//   (crop % 8 == 0, so flipping the container and pooling commute).
//
// Sparse planes and the dense arg-max: scores are >= 0 and an absent plane is all zero.  Starting from (value 0, plane 0) and letting a
// shipped plane win only when STRICTLY greater, in ascending plane id, gives np.argmax over the dense 21 planes: the lowest plane among the
// maxima, and plane 0 when every mean is 0 whether or not plane 0 was shipped.
#include "common.h"

namespace {

constexpr int CELLS_PER_WG = 32;      // 256 threads, 8 per cell

__global__ __launch_bounds__(256) void aff_labels_kernel(const wseg_aff_label_desc* __restrict__ descs, int crop, unsigned char* __restrict__ out) {
  const wseg_aff_label_desc d = descs[blockIdx.y];
  const int side = crop >> 3, cells = side * side;
  const int cell = blockIdx.x * CELLS_PER_WG + (threadIdx.x >> 3), row = threadIdx.x & 7;
  const int c = cell < cells ? cell : cells - 1;            // lanes past the end stay in the exchanges and store nothing
  const int oy = c / side, ox = c - oy * side;
  const int ux = d.flip ? side - 1 - ox : ox;               // cell column of the unflipped container
  const int py = oy * 8 + row - d.cont_top;                 // window row / first window column inside the pasted rectangle
  const int px = ux * 8 - d.cont_left;
  const bool row_in = py >= 0 && py < d.ch;
  const long first = row_in ? (long)(py + d.img_top) * d.W + (px + d.img_left) : 0;      // (+ j: read only where 0 <= px + j < cw)
  float best[2];
  int arg[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    best[s] = 0.f; arg[s] = 0;
    for (int k = 0; k < d.np[s]; ++k) {
      const float* plane = d.planes[s] + (long)k * d.plane_stride;
      float sum = 0.f;
      if (row_in) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (px + j >= 0 && px + j < d.cw) sum += plane[first + j];
      }
      sum += __shfl_xor(sum, 1, 64);
      sum += __shfl_xor(sum, 2, 64);
      sum += __shfl_xor(sum, 4, 64);
      const float mean = sum * 0.015625f;                   // / 64: exact
      if (mean > best[s]) { best[s] = mean; arg[s] = d.ids[s][k]; }
    }
  }
  int label = arg[0];
  if (arg[0] == 0) label = 255;
  if (arg[1] == 0) label = 0;
  if (fmaxf(best[0], best[1]) < 1e-5f) label = 255;
  if (row == 0 && cell < cells) out[(long)blockIdx.y * cells + cell] = (unsigned char)label;
}

}  // namespace

extern "C" size_t wseg_sizeof_aff_label_desc(void) { return sizeof(wseg_aff_label_desc); }

extern "C" int wseg_aff_labels_batch(const wseg_aff_label_desc* descs_dev, int n, int crop, unsigned char* out_u8, void* stream) {
  WSEG_CHECK(descs_dev && out_u8 && n > 0 && n <= 65535, "aff_labels_batch: bad arguments");
  WSEG_CHECK(crop >= 8 && crop % 8 == 0 && crop <= 32768, "aff_labels_batch: crop %d is no multiple of 8 in [8, 32768]", crop);
  const int cells = (crop / 8) * (crop / 8);
  hipLaunchKernelGGL(aff_labels_kernel, dim3((unsigned)((cells + CELLS_PER_WG - 1) / CELLS_PER_WG), n), dim3(256), 0, (hipStream_t)stream,
                     descs_dev, crop, out_u8);
  WSEG_LAUNCH_CHECK();
  return 0;
}
