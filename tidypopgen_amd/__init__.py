"""tidypopgen's genotype-matrix hot path, MI355X-native (HIP kernels behind a C ABI).

`import tidypopgen_amd` needs the built shared library (tidypopgen_amd/libtpg_hip.so);
there is no CPU fallback.  See DESIGN.md and INTEGRATION.md.
"""
from . import _lib  # noqa: F401  (raises ImportError if the HIP library is missing)
from .api import *  # noqa: F401,F403
from .api import (CODE_012, CODE_IMPUTE_PRED, FBM, Comm, Context, Multi, Pairwise, Roh, ShardedPairwise, View, default_context)  # noqa: F401
from .api import ibd_genome_length, ibd_segments, pairwise_ibd  # noqa: F401
from .api import fst_perm_labels, fst_perm_pvalue, fst_relabel_sums, pairwise_pop_fst_test  # noqa: F401
from .api import DeviceMatrix, amova_from_sums, amova_perm_labels, class_sums, gt_amova, pairwise_sqdist  # noqa: F401
from .api import (great_circle_dist, gt_mantel, mantel_from_sums, mantel_partial, mantel_pass_rows, mantel_perms, mantel_scratch_bytes,  # noqa: F401
                  mantel_sums, offdiag_center, offdiag_midranks, offdiag_moments)
from .api import gt_hclust, gt_nj, hclust_dist, hclust_order, nj, nj_edges, nj_newick  # noqa: F401
