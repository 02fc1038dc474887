// The discriminant analysis of DAPC (tidypopgen_amd/csrc/host/host_lda.h) as a stand-alone program for the host sanitizers
// (tests/test_dapc_host.py).  Reads "n d G n_da", the n x d scores (column-major, hexadecimal bit patterns) and the n group
// labels from the file named on the command line; prints "rc <code>" and, when the analysis ran, "dims L n_da" and one line of
// bit patterns per output (assign as integers), then "ok lda".  Every output is a heap array of exactly the documented size.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host/host_lda.h"

static void dump(const char* name, const std::vector<double>& a, size_t count) {
  printf("%s", name);
  for (size_t t = 0; t < count; t++) {
    uint64_t u;
    memcpy(&u, &a[t], sizeof u);
    printf(" %016" PRIx64, u);
  }
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 3;
  long long n;
  int d, G, n_da;
  if (fscanf(f, "%lld %d %d %d", &n, &d, &G, &n_da) != 4 || n < 1 || d < 1 || d > 64 || G < 1) return 4;
  std::vector<double> X((size_t)n * d);
  std::vector<int32_t> grp((size_t)n);
  for (double& x : X) {
    uint64_t u;
    if (fscanf(f, "%" SCNx64, &u) != 1) return 5;
    memcpy(&x, &u, sizeof x);
  }
  for (int32_t& g : grp) {
    int v;
    if (fscanf(f, "%d", &v) != 1) return 5;
    g = v;
  }
  fclose(f);
  const size_t Lmax = (size_t)(G < 2 ? 1 : (d < G - 1 ? d : G - 1)), N = (size_t)n, Gs = (size_t)G, D = (size_t)d;
  std::vector<double> prior(Gs), means(Gs * D), mu(D), scaling(D * Lmax), svd(Lmax), ind(N * Lmax), gc(Gs * Lmax), post(N * Gs);
  std::vector<int32_t> assign(N);
  int32_t L = 0, nda = 0;
  const char* why = "";
  const int rc = host_lda(X.data(), n, d, grp.data(), G, n_da, prior.data(), means.data(), mu.data(), scaling.data(), svd.data(), &L, &nda,
                          ind.data(), gc.data(), post.data(), assign.data(), &why);
  printf("rc %d %s\n", rc, why);
  if (rc == HOST_LDA_OK) {
    printf("dims %d %d\n", (int)L, (int)nda);
    dump("prior", prior, Gs);
    dump("means", means, Gs * D);
    dump("mu", mu, D);
    dump("scaling", scaling, D * (size_t)L);
    dump("svd", svd, (size_t)L);
    dump("ind_coord", ind, N * (size_t)nda);
    dump("grp_coord", gc, Gs * (size_t)nda);
    dump("posterior", post, N * Gs);
    printf("assign");
    for (size_t i = 0; i < N; i++) printf(" %d", (int)assign[i]);
    printf("\n");
  }
  printf("ok lda\n");
  return 0;
}
