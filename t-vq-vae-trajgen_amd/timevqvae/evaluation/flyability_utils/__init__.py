"""The numerical core of the reference's evaluation/flyability_utils: the trajectory
distances, on the device (csrc/tvq_traj.hip).  The BlueSky simulation, `traffic`, filtering
and plotting halves are out of scope, and so is the continuous `frechet`."""
from .trajectory_distances import (COLUMNS, discret_frechet, e_dtw, e_edr, e_erp, e_hausdorff,
                                   e_lcss, e_sspd, s_dtw, s_edr, s_erp, s_hausdorff, s_lcss,
                                   s_sspd, trajectory_distances_device)

__all__ = ["COLUMNS", "discret_frechet", "e_dtw", "e_edr", "e_erp", "e_hausdorff", "e_lcss",
           "e_sspd", "s_dtw", "s_edr", "s_erp", "s_hausdorff", "s_lcss", "s_sspd",
           "trajectory_distances_device"]
