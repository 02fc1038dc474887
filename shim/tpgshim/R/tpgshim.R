# tpgshim: R side.  The native wrappers of tidypopgen (R/RcppExports.R:4-91 there) are one-line functions of the form
#   increment_ibs_counts <- function(k, k2, genotype0, genotype1, genotype2, BM, rowInd, colInd)
#     invisible(.Call(`_tidypopgen_increment_ibs_counts`, k, k2, genotype0, genotype1, genotype2, BM, rowInd, colInd))
# tpg_enable() replaces them, inside tidypopgen's namespace, by the same one-liners bound to THIS package's symbols of the
# same names; tpg_disable() puts the originals back.  Nothing else of tidypopgen changes.

.tpg_routines <- c(
  alt_freq_dip_pseudo_cpp = 6L, fbm256_prod_and_rowSumsSq = 6L, grouped_alt_freq_dip_pseudo_cpp = 8L,
  grouped_missingness_cpp = 6L, grouped_summaries_dip_pseudo_cpp = 7L, gt_grouped_pi_diploid = 6L, gt_ind_hetero = 4L,
  gt_pi_diploid = 4L, pairwise_fst_hudson_loop = 6L, pairwise_fst_nei87_loop = 7L, pairwise_fst_wc84_loop = 6L,
  increment_as_counts = 7L, increment_ibs_counts = 8L, increment_king_numerator = 9L
)
.tpg_saved <- new.env()
# the Hardy-Weinberg wrappers (tpg_rshim_entries_hwe[] of the shim), rebound like the others
.tpg_routines_hwe <- c(SNPHWE2_R = 4L, hwe_on_matrix = 2L, gt_grouped_hwe = 6L)

tpg_enable <- function() {
  ns <- asNamespace("tidypopgen")
  routines <- c(.tpg_routines, .tpg_routines_hwe)
  for (name in names(routines)) {
    original <- get(name, envir = ns)
    if (is.null(.tpg_saved[[name]])) assign(name, original, envir = .tpg_saved)
    sym <- getNativeSymbolInfo(paste0("_tidypopgen_", name), PACKAGE = "tpgshim")
    stopifnot(length(formals(original)) == routines[[name]])
    replacement <- original
    body(replacement) <- bquote(.Call(.(sym), ..(lapply(names(formals(original)), as.name))), splice = TRUE)
    unlockBinding(name, ns)
    assign(name, replacement, envir = ns)
    lockBinding(name, ns)
  }
  invisible(TRUE)
}

tpg_disable <- function() {
  ns <- asNamespace("tidypopgen")
  for (name in ls(.tpg_saved)) {
    unlockBinding(name, ns)
    assign(name, get(name, envir = .tpg_saved), envir = ns)
    lockBinding(name, ns)
  }
  invisible(TRUE)
}

# only needed under TPG_RSHIM_DEFERRED=1 (then: after the block loop of snp_ibs / snp_king / snp_allele_sharing)
tpg_flush <- function() invisible(.Call(`_tidypopgen_tpg_flush`))
tpg_release <- function() invisible(.Call(`_tidypopgen_tpg_release`))
# only needed under TPG_RSHIM_CACHE=1 (an HBM copy of the whole FBM kept between calls): after anything that writes to X
tpg_invalidate <- function(X) invisible(.Call(`_tidypopgen_tpg_invalidate`, X))

# gt_impute_simple on the GPU: what R/gt_impute_simple.R does around bigsnpr::snp_fastImputeSimple, with the write to the
# FBM done by the library in place (missing byte 3 -> 4 + fill).  method "mode" | "mean0" | "random"; `seed` keys the random
# draws (R's generator is not used).  x is a gen_tibble; the result is x, imputed, with the imputed codes switched off.
tpg_gt_impute_simple <- function(x, method = c("mode", "mean0", "random"), seed = 0) {
  method <- match.arg(method)
  X <- attr(x$genotypes, "fbm")
  if (nrow(attr(x$genotypes, "loci")) != ncol(X)) {
    stop("The number of SNPs in the gen_tibble does not match the number of columns in the file backing matrix. ",
         "Before imputing, use gt_update_backingfile to update your file backing matrix.")
  }
  if (!is.null(attr(x$genotypes, "imputed"))) stop("object x is already imputed; use `gt_set_imputed(x, set = TRUE)`")
  if (!identical(X$code256, bigsnpr::CODE_012)) {
    if (identical(X$code256, bigsnpr::CODE_IMPUTE_PRED) || identical(X$code256, bigsnpr::CODE_DOSAGE)) {
      stop("object x is already imputed, but attr(x, 'imputed') is null")
    }
    stop("object x uses a code256 that is not compatible with imputation")
  }
  report <- .Call(`_tidypopgen_tpg_impute_simple`, X, match(method, c("mode", "mean0", "random")), as.numeric(seed))
  X$code256 <- bigsnpr::CODE_IMPUTE_PRED
  attr(x$genotypes, "fbm") <- X
  attr(x$genotypes, "imputed") <- "simple"
  attr(x$genotypes, "tpg_impute_report") <- c(imputed = report[1], loci_all_missing = report[2])
  tidypopgen::gt_set_imputed(x, set = FALSE)
  x
}

# loci_hwe of an ungrouped gen_tibble column in one call (R/loci_hwe.R:74-89: big_counts + hwe_on_matrix per block); X is
# the FBM.code256, ind.row / ind.col the kept individuals and loci.  gt_grouped_hwe, hwe_on_matrix and SNPHWE2_R keep their
# names and arguments: the shim registers them under the reference's own symbols (tpg_rshim_entries_hwe[]).
tpg_loci_hwe <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), mid_p = TRUE) {
  .Call(`_tidypopgen_tpg_loci_hwe`, X, as.integer(ind.row), as.integer(ind.col), isTRUE(mid_p))
}

# LD clumping of the loci ind.col in one call (the bigsnpr::snp_clumping call of R/loci_ld_clump.R:161-174; include/tpg.h
# "LD clumping" is the definition).  infos.chr / infos.pos describe the loci of ind.col, which must be ordered; exclude =
# positions in ind.col never to keep.  Returns a logical per locus of ind.col.  A missing genotype is an error.
tpg_ld_clump <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), infos.chr,
                         infos.pos = NULL, S = NULL, thr.r2 = 0.2, size = 100 / thr.r2, exclude = NULL) {
  m <- length(ind.col)
  hi <- integer(m)
  for (idx in split(seq_len(m), infos.chr)) {
    if (any(diff(idx) != 1L)) stop("loci are not ordered: a chromosome appears in more than one run")
    if (is.null(infos.pos)) {
      hi[idx] <- pmin(idx + floor(size), idx[length(idx)])
    } else {
      p <- infos.pos[idx]
      if (is.unsorted(p)) stop("loci are not ordered: positions decrease inside a chromosome")
      hi[idx] <- idx[1] - 1L + findInterval(p + size * 1000, p)
    }
  }
  ex <- NULL
  if (length(exclude) > 0) {
    ex <- logical(m)
    ex[exclude] <- TRUE
  }
  .Call(`_tidypopgen_tpg_ld_clump`, X, as.integer(ind.row), as.integer(ind.col), hi, as.numeric(thr.r2),
        if (is.null(S)) NULL else as.numeric(S), ex)
}

# runs of homozygosity of every individual in one call (the loop of R/windows_indiv_roh.R:129-143 around
# detectRUNS::slidingRuns; include/tpg.h "Runs of homozygosity" is the definition).  chromosome / position describe the loci of
# ind.col, which must be ordered.  Returns a data.frame with one row per run: indiv (position in ind.row), nSNP, from, to,
# lengthBps, first, last (positions in ind.col).
tpg_indiv_roh <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), chromosome, position,
                          window_size = 15, threshold = 0.05, min_snp = 3, heterozygosity = FALSE, max_opp_window = 1,
                          max_miss_window = 1, max_gap = 10^6, min_length_bps = 1000, min_density = 1 / 1000,
                          max_opp_run = NULL, max_miss_run = NULL) {
  params <- c(window_size, threshold, min_snp, as.numeric(heterozygosity), max_opp_window, max_miss_window, max_gap,
              min_length_bps, min_density, if (is.null(max_opp_run)) NA_real_ else max_opp_run,
              if (is.null(max_miss_run)) NA_real_ else max_miss_run)
  as.data.frame(.Call(`_tidypopgen_tpg_indiv_roh`, X, as.integer(ind.row), as.integer(ind.col),
                      as.integer(factor(chromosome, levels = unique(chromosome))), as.numeric(position), as.numeric(params)))
}

# Tajima's D per group in one call (the big_apply and the loop over groups of R/pop_tajimas_d.R:113-147; include/tpg.h
# "Tajima's D" is the definition).  group_ids0 = dplyr::group_indices(.x) - 1, or NULL for one group of everybody.
tpg_pop_tajimas_d <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), group_ids0 = NULL,
                              n_groups = 1L) {
  .Call(`_tidypopgen_tpg_pop_tajimas_d`, X, as.integer(ind.row), as.integer(ind.col), group_ids0, as.integer(n_groups))
}

# Tajima's D per window and group in one call (loci_pi and the runner call per group of R/windows_pop_tajimas_d.R:80-103).
# lo / hi: 0-based half-open ranges of positions in ind.col, one per window; pad_na: the windows runner pads under complete =
# TRUE (NULL: none).  Returns list(stat, n_loci), windows x groups each.
tpg_windows_pop_tajimas_d <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X),
                                      group_ids0 = NULL, n_groups = 1L, lo, hi, pad_na = NULL, min_loci = 1L) {
  .Call(`_tidypopgen_tpg_windows_pop_tajimas_d`, X, as.integer(ind.row), as.integer(ind.col), group_ids0,
        as.integer(n_groups), lo, hi, pad_na, as.integer(min_loci))
}

# Windowed pairwise Fst in one call that never forms the by-locus matrices (pairwise_pop_fst(return_num_dem = TRUE) and the two
# windows_stats_generic calls of R/windows_pairwise_pop_fst.R:62-107; include/tpg.h "windowed pairwise Fst" is the definition).
# group_ids0 = dplyr::group_indices(.x) - 1; method 0 = Hudson (what the reference takes here), 1 = Nei87, 2 = WC84; lo / hi /
# pad_na as tpg_windows_pop_tajimas_d takes them.  Returns the windows x pairs matrix, pairs in utils::combn(n_groups, 2) order.
tpg_windows_pairwise_pop_fst <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), group_ids0,
                                         n_groups, method = 0L, lo, hi, pad_na = NULL, min_loci = 1L) {
  .Call(`_tidypopgen_tpg_windows_pairwise_pop_fst`, X, as.integer(ind.row), as.integer(ind.col), group_ids0,
        as.integer(n_groups), as.integer(method), lo, hi, pad_na, as.integer(min_loci))
}

# Windowed PBS of every triplet of populations from that windowed Hudson Fst (R/windows_nwise_pop_pbs.R:78-114); the window Fst
# stays on the device in between.  Returns list(pbs, fst): pbs windows x 6 per triplet of utils::combn(n_groups, 3) (pbs_1,
# pbs_2, pbs_3, pbsn1_1, pbsn1_2, pbsn1_3), fst the windows x pairs matrix or NULL unless return_fst.
tpg_windows_nwise_pop_pbs <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), group_ids0,
                                      n_groups, lo, hi, pad_na = NULL, min_loci = 1L, return_fst = FALSE) {
  .Call(`_tidypopgen_tpg_windows_nwise_pop_pbs`, X, as.integer(ind.row), as.integer(ind.col), group_ids0,
        as.integer(n_groups), lo, hi, pad_na, as.integer(min_loci), isTRUE(return_fst))
}

# Blocked f2 and allele-frequency products in one call (gt_to_aftable, admixtools' discard_from_aftable and afs_to_f2_blocks of
# R/gt_extract_f2.R:141-189; include/tpg.h "f2 blocks" is the definition).  lo / hi: 0-based half-open ranges of positions in
# ind.col, one per jackknife block; ploidy = NULL: all diploid; keep: NULL or one logical per locus (transitions, transversions
# and outpop are filters on the locus table: fold them into keep).  Returns list(f2, counts, ap, ap_counts: groups x groups x
# blocks; block_lengths).
tpg_f2_blocks <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), group_ids0 = NULL,
                          n_groups = 1L, ploidy = NULL, lo, hi, maxmiss = 0, minmaf = 0, maxmaf = 0.5, minac2 = FALSE,
                          poly_only = c("f2"), apply_corr = TRUE, keep = NULL) {
  if (isTRUE(poly_only)) poly_only <- c("f2", "ap")
  if (isFALSE(poly_only)) poly_only <- character(0)
  if (!all(poly_only %in% c("f2", "ap"))) stop("poly_only: only 'f2' and 'ap' are supported")
  if (!(isTRUE(minac2) || isFALSE(minac2))) stop("minac2 must be TRUE or FALSE (admixtools' minac2 = 2 is not supported)")
  params <- c(maxmiss, minmaf, maxmaf, as.numeric(minac2), sum(c(f2 = 1, ap = 2)[unique(poly_only)]), as.numeric(apply_corr),
              if (is.null(keep)) numeric(0) else as.numeric(as.logical(keep)))
  .Call(`_tidypopgen_tpg_f2_blocks`, X, as.integer(ind.row), as.integer(ind.col), group_ids0, as.integer(n_groups), ploidy,
        lo, hi, params)
}

# Ancestry proportions by EM on the GPU for one k and one run (the PLINK export, the outside `admixture` program and the reading
# back of its .Q / .P files of R/gt_admixture.R:86-236; include/tpg.h "admixture" is the definition).  seed: one whole number;
# q0 / p0: a start (individuals x k, loci x k) or NULL for the seeded one.  Returns the gt_admix list of the reference for that
# run (k, Q, P, loglik), with n_iter and converged beside it.  P is the frequency of the counted (alt) allele.
# crossval = TRUE adds cv, the name the reference uses: the cv_folds-fold cross-validation error of this k from the same start
# (include/tpg.h "admixture cross-validation"; cv_seed, one whole number, keys the folds).
# conda_env and outdir have no counterpart.
gt_admixture_gpu <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), k, seed = 0,
                             max_iter = 1000L, tol = 1e-4, q0 = NULL, p0 = NULL, crossval = FALSE, cv_folds = 5L, cv_seed = 0) {
  res <- .Call(`_tidypopgen_tpg_admixture`, X, as.integer(ind.row), as.integer(ind.col), as.integer(k), as.numeric(seed),
               as.integer(max_iter), as.numeric(tol), q0, p0)
  adm_list <- list(k = as.integer(k), Q = list(res$Q), P = list(res$P), loglik = res$loglik, n_iter = res$n_iter,
                   converged = res$converged)
  if (isTRUE(crossval)) {
    cvres <- .Call(`_tidypopgen_tpg_admixture_cv`, X, as.integer(ind.row), as.integer(ind.col), as.integer(k), as.numeric(seed),
                   as.integer(max_iter), as.numeric(tol), q0, p0, as.integer(cv_folds), as.numeric(cv_seed))
    adm_list$cv <- cvres$cv_error
  }
  class(adm_list) <- c("gt_admix", "list")
  adm_list
}

# gt_admixture_gpu with the EM under squared extrapolation (include/tpg.h "admixture, accelerated"): the same likelihood, the same
# arguments and the same list, reached in fewer EM steps; n_iter still counts EM steps, and n_cycles and n_rejected (the
# extrapolation cycles, and those of them that were rejected) sit beside it.  crossval = TRUE refits every fold the same way.
gt_admixture_squarem_gpu <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), k, seed = 0,
                                     max_iter = 1000L, tol = 1e-4, q0 = NULL, p0 = NULL, crossval = FALSE, cv_folds = 5L,
                                     cv_seed = 0) {
  res <- .Call(`_tidypopgen_tpg_admixture_squarem`, X, as.integer(ind.row), as.integer(ind.col), as.integer(k), as.numeric(seed),
               as.integer(max_iter), as.numeric(tol), q0, p0)
  adm_list <- list(k = as.integer(k), Q = list(res$Q), P = list(res$P), loglik = res$loglik, n_iter = res$n_iter,
                   converged = res$converged, n_cycles = res$n_cycles, n_rejected = res$n_rejected)
  if (isTRUE(crossval)) {
    cvres <- .Call(`_tidypopgen_tpg_admixture_cv_squarem`, X, as.integer(ind.row), as.integer(ind.col), as.integer(k),
                   as.numeric(seed), as.integer(max_iter), as.numeric(tol), q0, p0, as.integer(cv_folds), as.numeric(cv_seed))
    adm_list$cv <- cvres$cv_error
  }
  class(adm_list) <- c("gt_admix", "list")
  adm_list
}

# Ancestry proportions by sparse non-negative matrix factorisation on the GPU for one k and one run (the .geno export and the
# LEA::snmf run of R/gt_snmf.R; include/tpg.h "sNMF" is the definition).  seed: one whole number; q0: a start (individuals x k) or
# NULL for the seeded one.  entropy = TRUE holds a share `percentage` of the typed genotypes out, fits on the rest, as LEA does, and
# adds cv (the masked cross-entropy, the name the reference uses) and cv_all.  Returns the gt_admix list of the reference for that
# run (k, Q, P, G, algorithm), with ls, n_iter and converged beside it.  project, I and ploidy have no counterpart.
gt_snmf_gpu <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), k, alpha = 10,
                        tolerance = 1e-5, entropy = FALSE, percentage = 0.05, iterations = 200L, seed = 0, q0 = NULL) {
  res <- .Call(`_tidypopgen_tpg_snmf`, X, as.integer(ind.row), as.integer(ind.col), as.integer(k), as.numeric(alpha),
               as.numeric(tolerance), as.integer(iterations), as.numeric(seed), if (isTRUE(entropy)) as.numeric(percentage) else NULL,
               q0)
  adm_list <- list(k = as.integer(k), Q = list(res$Q), P = list(res$P), G = list(res$G), ls = res$ls, n_iter = res$n_iter,
                   converged = res$converged, algorithm = "SNMF")
  if (isTRUE(entropy)) {
    adm_list$cv <- res$cv
    adm_list$cv_all <- res$cv_all
  }
  class(adm_list) <- c("gt_admix", "list")
  adm_list
}

# Clusters on PCA scores on the GPU (R/gt_cluster_pca.R:75-177; include/tpg.h "k-means on PCA scores" is the definition: Lloyd's
# algorithm from seeded start rows in the place of stats::kmeans, every run of every k in one batch).  x: a gt_pca object;
# seed: one whole number.  Returns the reference's gt_cluster_pca object (clusters$method, n_pca, k, WSS, AIC, BIC, groups), with
# n_iter, converged and n_empty of the winning runs beside them, so gt_cluster_pca_best_k() and gt_dapc() run on it unchanged.
# method = "ward" is gt_cluster_pca_ward_gpu below.
gt_cluster_pca_gpu <- function(x, n_pca = NULL, k_clusters = c(1, round(nrow(x$u) / 10)), n_iter = 1e5, n_start = 10, seed = 0) {
  if (is.null(x) || !inherits(x, "gt_pca")) stop("'x' should be a 'gt_pca' object")
  n <- nrow(x$u)
  if (is.null(n_pca)) n_pca <- length(x$d)
  if (length(k_clusters) == 1) {
    nb_clust <- k_clusters
  } else if (length(k_clusters) == 2) {
    nb_clust <- k_clusters[1]:k_clusters[2]
  } else {
    stop("'k_clusters' should be either a single value, or the minimum and maximum to be tested")
  }
  x_scores <- sweep(x$u, 2, x$d, "*")[, seq_len(n_pca), drop = FALSE]
  res <- .Call(`_tidypopgen_tpg_cluster_pca`, x_scores, as.numeric(nb_clust), as.integer(n_start), as.integer(n_iter),
               as.numeric(seed))
  groups <- lapply(seq_along(nb_clust), function(i) stats::setNames(res$groups[, i], rownames(x$u)))
  names(groups) <- nb_clust
  x$clusters <- list(method = "kmeans", n_pca = n_pca, k = nb_clust, WSS = res$WSS,
                     AIC = n * log(res$WSS / n) + 2 * nb_clust, BIC = n * log(res$WSS / n) + log(n) * nb_clust,
                     groups = groups, n_iter = res$n_iter, converged = res$converged, n_empty = res$n_empty)
  class(x) <- c("gt_cluster_pca", class(x))
  x
}

# method = "ward" of gt_cluster_pca on the GPU (R/gt_cluster_pca.R:156-169; include/tpg.h "Ward clustering on PCA scores" is the
# definition): ONE tree, cut at every k, in the place of one stats::hclust per k.  criterion = "reference" is the reference's
# hclust(dist(x)^2, "ward.D2"), Ward's recurrence on d^4; "ward" is the proper criterion, on d^2.  Returns the reference's
# gt_cluster_pca object with the tree's merge and height (as hclust reports them) beside the groups, so gt_cluster_pca_best_k()
# and gt_dapc() run on it unchanged.  hclust$order is not produced.  k goes up to 1024 (the limit of the WSS call): the default
# range passes that from 10 246 individuals on and is then an error before the tree is built; give k_clusters.
gt_cluster_pca_ward_gpu <- function(x, n_pca = NULL, k_clusters = c(1, round(nrow(x$u) / 10)), criterion = c("reference", "ward")) {
  if (is.null(x) || !inherits(x, "gt_pca")) stop("'x' should be a 'gt_pca' object")
  criterion <- match.arg(criterion)
  n <- nrow(x$u)
  if (is.null(n_pca)) n_pca <- length(x$d)
  if (length(k_clusters) == 1) {
    nb_clust <- k_clusters
  } else if (length(k_clusters) == 2) {
    nb_clust <- k_clusters[1]:k_clusters[2]
  } else {
    stop("'k_clusters' should be either a single value, or the minimum and maximum to be tested")
  }
  x_scores <- sweep(x$u, 2, x$d, "*")[, seq_len(n_pca), drop = FALSE]
  res <- .Call(`_tidypopgen_tpg_cluster_pca_ward`, x_scores, as.numeric(nb_clust), if (criterion == "reference") 2L else 1L)
  groups <- lapply(seq_along(nb_clust), function(i) stats::setNames(res$groups[, i], rownames(x$u)))
  names(groups) <- nb_clust
  x$clusters <- list(method = "ward", criterion = criterion, n_pca = n_pca, k = nb_clust, WSS = res$WSS,
                     AIC = n * log(res$WSS / n) + 2 * nb_clust, BIC = n * log(res$WSS / n) + log(n) * nb_clust,
                     groups = groups, merge = res$merge, height = res$height)
  class(x) <- c("gt_cluster_pca", class(x))
  x
}

# PCA-based genome scan on the GPU (R/gt_pcadapt.R:44-86 around bigsnpr::snp_pcadapt; include/tpg.h "pcadapt" is the definition).
# U.row: the first k columns of the PCA's u for the rows ind.row.  Returns the reference's object: a data.frame(score) of class
# "mhtest" whose `predict` attribute gives log10 p-values from the chi-square with k degrees of freedom; dist, the device's own
# log10p and the genomic-control factor ride along as attributes.
gt_pcadapt_gpu <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), U.row) {
  U.row <- as.matrix(U.row)
  if (nrow(U.row) != length(ind.row)) stop("U.row must have one row per element of ind.row")
  K <- ncol(U.row)
  storage.mode(U.row) <- "double"
  res <- .Call(`_tidypopgen_tpg_pcadapt`, X, as.integer(ind.row), as.integer(ind.col), U.row)
  fun.pred <- function(xtr) stats::pchisq(xtr, df = K, lower.tail = FALSE, log.p = TRUE) / log(10)
  structure(data.frame(score = res$score), class = c("mhtest", "data.frame"), transfo = identity, predict = fun.pred,
            dist = res$dist, log10p = res$log10p, gc_lambda = res$gc_lambda)
}

# PCA with removal of long-range LD regions on the GPU (R/gt_pca_autoSVD.R around bigsnpr::snp_autoSVD; include/tpg.h "autoSVD" is
# the definition).  infos.chr / infos.pos describe the loci of ind.col, in order; thr.r2 = NA skips clumping; size is the clumping
# window in kb (in loci without positions).  Returns the big_SVD list with attr(, "subset") (the kept loci, as positions in the
# FBM) and attr(, "lrldr") (a data.frame Chr / Start / Stop, only with positions), as bigsnpr does.
gt_pca_autoSVD_gpu <- function(X, infos.chr, infos.pos = NULL, ind.row = bigstatsr::rows_along(X),
                               ind.col = bigstatsr::cols_along(X), k = 10L, thr.r2 = 0.2, size = 100 / thr.r2, roll.size = 50L,
                               int.min.size = 20L, alpha.tukey = 0.05, min.mac = 10L, max.iter = 5L) {
  chr <- as.integer(factor(infos.chr, levels = unique(infos.chr)))
  if (length(chr) != length(ind.col)) stop("infos.chr must have one entry per element of ind.col")
  hi <- NULL
  if (!is.na(thr.r2)) {
    hi <- numeric(length(chr))
    for (idx in split(seq_along(chr), chr)) {
      hi[idx] <- if (is.null(infos.pos)) pmin(idx + floor(size), max(idx)) - 1
                 else min(idx) + findInterval(infos.pos[idx] + size * 1000, infos.pos[idx]) - 2
    }
  }
  params <- c(k, if (is.na(thr.r2)) 0 else thr.r2, roll.size, int.min.size, alpha.tukey, min.mac, max.iter)
  res <- .Call(`_tidypopgen_tpg_pca_auto_svd`, X, as.integer(ind.row), as.integer(ind.col), chr,
               if (is.null(infos.pos)) NULL else as.numeric(infos.pos), hi, as.numeric(params))
  lr <- attr(res, "lrldr")
  out <- structure(res[c("d", "u", "v", "center", "scale")], class = "big_SVD", subset = ind.col[attr(res, "subset")],
                   lrldr = data.frame(Chr = unique(infos.chr)[lr$Chr], Start = lr$Start, Stop = lr$Stop),
                   n_iter = res$n_iter, converged = res$converged)
  out
}

# whole analyses on every GPU of the node (TPG_DEVICES); X is the FBM.code256 of a gen_tibble (attr(x$genotypes, "fbm"))
# which: the matrices wanted; only the cross-products they need are computed (GRM alone: 2 of 5, KING + GRM: 4 of 5)
tpg_snp_pairwise <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X),
                             adjusted_counts = FALSE, which = c("ibs", "king", "allele_sharing", "grm")) {
  which <- match.arg(which, several.ok = TRUE)
  mask <- sum(c(ibs = 1L, king = 2L, allele_sharing = 4L, grm = 8L)[unique(which)])
  .Call(`_tidypopgen_tpg_snp_pairwise`, X, as.integer(ind.row), as.integer(ind.col), adjusted_counts, as.integer(mask))
}
tpg_grouped_alt_freq <- function(X, ind.row, ind.col, group_ids0 = NULL, n_groups = 0L, ploidy, as_counts = FALSE) {
  .Call(`_tidypopgen_tpg_grouped_alt_freq`, X, as.integer(ind.row), as.integer(ind.col), group_ids0, as.integer(n_groups),
        as.numeric(ploidy), as_counts)
}
tpg_pairwise_pop_fst <- function(X, ind.row, ind.col, group_ids0, n_groups, ploidy,
                                 method = c("Hudson", "Nei87", "WC84"), pairwise_combn = utils::combn(n_groups, 2),
                                 by_locus = FALSE, return_num_dem = FALSE) {
  method <- match(match.arg(method), c("Hudson", "Nei87", "WC84")) - 1L
  .Call(`_tidypopgen_tpg_pairwise_pop_fst`, X, as.integer(ind.row), as.integer(ind.col), as.integer(group_ids0),
        as.integer(n_groups), as.numeric(ploidy), method, pairwise_combn, by_locus, return_num_dem)
}
tpg_pca_partial_svd <- function(X, ind.row = bigstatsr::rows_along(X), ind.col = bigstatsr::cols_along(X), k = 10L) {
  .Call(`_tidypopgen_tpg_pca_partial_svd`, X, as.integer(ind.row), as.integer(ind.col), as.integer(k))
}
