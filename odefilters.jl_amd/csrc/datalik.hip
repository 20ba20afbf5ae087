// Data log-likelihood of noisy observations per trajectory (datalik.h).  One lane per trajectory sweeps the
// filter records of a fixed grid backwards; the time axis is a recursion, so there is one launch, no chunking and no fold.  The
// kernels depend on (d, q) only and are instantiated here once, for the compiled-in and the run-time compiled fields alike.
#include "datalik_host.h"

namespace odef {

bool datalik_has(int d, int q) { return has_dq<kDataLikMaxD, kDataLikMaxState>(d, q); }

int datalik_run(DataLikState& st, const DataLikRequest& r, hipStream_t stream, float* ms, int* n_launches, char* kname, size_t kname_n,
                std::string& err) {
  st.valid = false;
  if (!datalik_has(r.d, r.q)) return pass_fail(err, "data log-likelihood: no kernel for (d, q) = (%d, %d)", r.d, r.q);
  const DataLikWhen<long long> when{(const long long*)r.obs_save, r.save_bytes, (size_t)r.n_save, "ODEF_L_OBS_SAVE", "1 .. n_save int64",
                                    "saves"};
  auto check_saves = [&](const long long* idx, size_t M, std::string& err) {
    for (size_t j = 0; j < M; ++j)
      if (idx[j] < 0 || idx[j] >= r.n_save || (j > 0 && idx[j] <= idx[j - 1]))
        return pass_fail(err, "data log-likelihood: observed saves must be strictly increasing within 0 .. n_save - 1 = %ld "
                              "(entry %zu is %lld)", r.n_save - 1, j, idx[j]);
    return 0;
  };
  DataLikArgs a;
  if (datalik_prepare(st, r, when, stream, check_saves, a, err)) return -1;
  a.ptab = r.ptab;
  a.tab_idx = r.tab_idx;
  a.hs = r.hs;
  a.obs_save = when.ptr;
  auto launch = [&]<int d, int q>() {
    hipLaunchKernelGGL((data_loglik_kernel<d, q>), dim3((unsigned)((a.N + kDataLikWave - 1) / kDataLikWave)), dim3(kDataLikWave), 0, stream,
                       a);
  };
  return datalik_launch<kDataLikMaxState>(st, r.d, r.q, launch, "data log-likelihood", "data_loglik_kernel", stream, ms, n_launches, kname,
                                          kname_n, err);
}

void datalik_free(DataLikState& st) {
  free_device(st.out[0], st.out[1]);
  st.timer.destroy();
  st = DataLikState{};
}

}  // namespace odef
