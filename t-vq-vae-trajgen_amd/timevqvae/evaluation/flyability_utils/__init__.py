"""The numerical core of the reference's evaluation/flyability_utils: the trajectory
distances, on the device (csrc/tvq_traj.hip, and csrc/tvq_traj_frechet.hip for the continuous
Frechet distance).  The BlueSky simulation, `traffic`, filtering and plotting halves are out
of scope.  The continuous distance is exported as `frechet_device` (a batch); the
reference's per-pair name `frechet` lives in `trajectory_distances` only."""
from .trajectory_distances import (COLUMNS, discret_frechet, e_dtw, e_edr, e_erp, e_hausdorff,
                                   e_lcss, e_sspd, frechet_device, s_dtw, s_edr, s_erp,
                                   s_hausdorff, s_lcss, s_sspd, trajectory_distances_device)

__all__ = ["COLUMNS", "discret_frechet", "e_dtw", "e_edr", "e_erp", "e_hausdorff", "e_lcss",
           "e_sspd", "frechet_device", "s_dtw", "s_edr", "s_erp", "s_hausdorff", "s_lcss",
           "s_sspd", "trajectory_distances_device"]
