// pf_workspace.h -- the layout of the PointFusion map step's workspace (e2e_pf_workspace_bytes), shared by the forward
// (pointfusion.hip) and the tape of its adjoint (pointfusion_grad.hip).
#pragma once
#include <stdint.h>

#define PF_T 256
#define PF_NONE 0xFFFFFFFFu
#define PF_KEY_NONE 0xFFFFFFFFFFFFFFFFull

// ordered stream compaction: CP_ITEMS items per thread, CP_BLOCK per workgroup
#define CP_ITEMS 4
#define CP_BLOCK (PF_T * CP_ITEMS)

// pix_key u64[N] | pix_best u32[N] | pix_of_point u32[cap] | counts u32[max(nbm,nbp)] | any_match u32[4] | flags u8[cap]
struct PfWs {
    unsigned long long* pix_key;
    unsigned int* pix_best;
    unsigned int* pix_of_point;
    unsigned int* counts;
    unsigned int* any_match;
    unsigned char* flags;
};
static inline PfWs pf_ws(void* ws, int64_t cap, int H, int W) {
    const int64_t N = (int64_t)H * W;
    const int64_t nbm = (cap + CP_BLOCK - 1) / CP_BLOCK + 1, nbp = (N + CP_BLOCK - 1) / CP_BLOCK + 1;
    PfWs w;
    char* p = (char*)ws;
    w.pix_key = (unsigned long long*)p; p += 8 * N;
    w.pix_best = (unsigned int*)p; p += 4 * N;
    w.pix_of_point = (unsigned int*)p; p += 4 * cap;
    w.counts = (unsigned int*)p; p += 4 * (nbm > nbp ? nbm : nbp);
    w.any_match = (unsigned int*)p; p += 16;
    w.flags = (unsigned char*)p;
    return w;
}
