// Test harness (g++): the segment-table arithmetic of csrc/pp_segments.h as the host compiles it, one C entry point per function.
#include "../../packppi_amd/csrc/pp_segments.h"

extern "C" int seg_of_row(const int32_t *off, int n_seg, int n) { return pp_seg_of_row(off, n_seg, n); }
extern "C" int seg_start(const int32_t *off, int s, int n) { return pp_seg_start(off, s, n); }
extern "C" void seg_rows(const int32_t *off, int s, int N, int *out) { pp_seg_rows(off, s, N, out[0], out[1]); }
// decoy groups: out = (consistent?, base, len, row0) of group g; the group of a consensus row; the first row of decoy d of group g
extern "C" void group_rows(const int32_t *off, int g, int D, int N, int *out) {
    out[0] = pp_group_rows(off, g, D, N, out[1], out[2], out[3]) ? 1 : 0;
}
extern "C" int group_of_cons_row(const int32_t *off, int G, int D, int N, int crow) { return pp_group_of_cons_row(off, G, D, N, crow); }
extern "C" int decoy_row0(const int32_t *off, int g, int D, int N, int d) { return pp_decoy_row0(off, g, D, N, d); }
// every row of a batch at once: out [N][2] = what k_fill_seg writes to pp_ctx::seg
extern "C" void seg_fill_all(const int32_t *off, int n_seg, int N, int max_len, int *out) {
    for (int n = 0; n < N; n++) pp_seg_fill(off, n_seg, N, max_len, n, out[2 * n], out[2 * n + 1]);
}
