"""redclust.jl_amd — MI355X-native Gibbs-sweep hot path of RedClust.jl behind the reference's
runsampler / MCMCData / MCMCOptionsList / MCMCResult surface.

The directory name is not a valid Python identifier; import it through the repo-root shim:

    import redclust_amd as rc
"""
from ._lib import Context, Comm, measure_read_ceiling, RedClustHIPError, RedClustDomainError, build, build_diag, lib, SIGNATURES  # noqa: F401
from .types import MCMCData, MCMCOptionsList, MCMCResult, MCMCState, PriorHyperparamsList, KmedoidsResult, KmeansResult  # noqa: F401
from .sampler import runsampler, sample_r, sample_p, iac_ess_acf  # noqa: F401
from .prior import fitprior, fitprior2, fitprior_kmeans, fitprior2_kmeans, kmeans, sampleK, sampledist, pmf, kmedoids, sample_rp, detectknee  # noqa: F401
from .datagen import generatemixture, oracle_coclustering, likelihood_hyperparams, likelihood_hyperparams_device  # noqa: F401
from .chains import chain_seed, merge_chains, run_chains, run_chains_single_process, library_merge, agreed_merge, device_counts_tensor  # noqa: F401
from .pointestimate import (getpointestimate, lossmatrix, binderloss, infodist, varinfo, evaluateclustering,  # noqa: F401
                            summarise, searchpointestimate, expectedloss, expectedvi, expectedid, cocluster_counts,
                            posterior_counts, posterior_coclustering, hclust, hclustpointestimate, expectedlosses,
                            linkage_matrix, leaf_order, partitiondistances, expecteddistances, credibleball,
                            credibleball_from_distances, relabel, Relabelling, expectedpear, pearfraction, expectedpears,
                            searchmaxpear, maxpear, expectedari)
from .wasabi import searchvigroups, wasabi, wasabi_scan, WasabiResult  # noqa: F401
from .predict import predict, predict_points, Prediction, predict_joint, JointPrediction  # noqa: F401
from .metrics import pairwise, METRICS  # noqa: F401
from .score import scorelabellings, loglik_from_blocks, mapestimate, searchmapestimate, reweight  # noqa: F401
from .profiles import clusterprofiles, ClusterProfiles, silhouettes_from_sums, exemplars  # noqa: F401
