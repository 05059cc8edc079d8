"""The numerical half of the reference's evaluation/flyability_eval.py:
`calculate_trajectory_distances` (:271-351) on plain arrays.

The reference walks two `traffic.Traffic` objects flight by flight and scores
`flight.data[["latitude", "longitude"]].values` of the generated flight against its simulated
counterpart with 14 host distances.  Here the caller passes those (n, 2) arrays directly and
the whole list is scored in one device batch (flyability_utils.trajectory_distances).  The
BlueSky simulation, `traffic`, filtering, plotting and the CLI are out of scope.  The 14th
distance, the continuous Frechet distance, is the costly one (a binary search over up to
2 n0 n1 critical values with a decision over the whole free-space diagram per probe) and is
opt-in: `frechet=True` adds the "Frechet" key, the default dict has the other 13."""
from typing import Dict, List

from .flyability_utils.trajectory_distances import (COLUMNS, frechet_device,
                                                    trajectory_distances_device)

EPS = 0.009  # flyability_eval.py:304, "1 km in degrees", for LCSS and EDR


def calculate_trajectory_distances(gen_trajs, sim_trajs, ADEP_lat: float, ADEP_lon: float,
                                   frechet: bool = False) -> Dict[str, List[float]]:
    """Distances between each generated trajectory and its simulated counterpart.

    gen_trajs, sim_trajs: equal-length lists of (n, 2) [latitude, longitude] arrays or tensors.
    As in the reference the rows go to the distance functions as they are (so the spherical
    ones read the latitude as their `lon`), the ERP gap point is (ADEP_lat, ADEP_lon), eps is
    0.009, spherical LCSS gets eps * 1e6 and spherical EDR eps.  Returns the reference's dict of
    lists of Python floats; with frechet=True "Frechet" (the continuous distance) is its last
    key, as in the reference, otherwise the key is absent."""
    gen_trajs, sim_trajs = list(gen_trajs), list(sim_trajs)
    out = trajectory_distances_device(gen_trajs, sim_trajs, (ADEP_lat, ADEP_lon), eps=EPS,
                                      lcss_spherical_eps=EPS * 1e6, edr_spherical_eps=EPS)
    cols = out.t().cpu().tolist()
    res = {name: cols[c] if cols else [] for c, name in enumerate(COLUMNS)}
    if frechet:
        res["Frechet"] = frechet_device(gen_trajs, sim_trajs, device=out.device).cpu().tolist()
    return res
