"""shadow_amd -- MI355X-native routing engine for Shadow's topology subsystem.

The product is ``libshdtopo.so`` (HIP kernels for gfx950 + C++ host runtime) behind the C ABI
in ``include/shd_topology_abi.h``; this package is the Python mirror of the reference's
topology interface (``topology.py``) and the one-process-per-GPU sharding driver
(``sharding.py``).  See DESIGN.md.
"""
from .topology import (CROSSING_DTYPE, Address, Random, RouteSchedule, Topology,  # noqa: F401
                       crossings_by_watch, ip_to_network, network_to_ip)

__all__ = ["Address", "Random", "Topology", "RouteSchedule", "ip_to_network", "network_to_ip",
           "crossings_by_watch", "CROSSING_DTYPE"]
