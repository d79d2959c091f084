"""Python facade over the C++ scheduling core.

Mirrors the reference's internal.SchedulerAlgorithm contract
(pkg/internal/types.go:57-100): Schedule, Add/Update/DeleteNode,
Add/DeleteUnallocatedPod, Add/DeleteAllocatedPod plus inspect getters.
The sequencing contract is the caller's job (HivedScheduler serializes calls).
"""
from __future__ import annotations

import threading
from typing import Dict, List

from . import hivedcore
from .api import constants
from .api.types import (
    Config,
    PodBindInfo,
    PodSchedulingSpec,
    WebServerError,
    dataclass_to_plain,
)

FILTERING = "Filtering"
PREEMPTING = "Preempting"


def normalize_spec(config: Config) -> dict:
    """Convert a parsed (and inferred) Config into the C++ core's spec dict."""
    pc = config.physicalCluster
    return {
        "cellTypes": {
            name: {
                "childCellType": ct.childCellType or "",
                "childCellNumber": ct.childCellNumber,
                "isNodeLevel": ct.isNodeLevel,
            }
            for name, ct in pc.cellTypes.items()
        },
        "physicalCells": [c.to_dict() for c in pc.physicalCells],
        "virtualClusters": {
            vc: {
                "virtualCells": [
                    {"cellType": v.cellType, "cellNumber": v.cellNumber} for v in spec.virtualCells
                ],
                "pinnedCells": [{"pinnedCellId": p.pinnedCellId} for p in spec.pinnedCells],
            }
            for vc, spec in config.virtualClusters.items()
        },
    }


# One of bind / preempt / wait: the core's native result type. Read-only
# attributes kind, bind_info (a PodBindInfo built on first access, None unless
# kind == "bind"), victim_node, victim_pod_keys and wait_reason.
ScheduleResult = hivedcore.ScheduleResult


class HivedAlgorithm:
    """Thread-safe wrapper: a single lock serializes all calls, matching the
    reference's algorithmLock (hived_algorithm.go:104).

    The one call per decision, `schedule_pod`, and the release of a pod by its
    key, `delete_allocated_pod_by_key`, are the exceptions: they are the core's
    own native methods, bound in __init__, with no Python frame, lock or `try`
    around them. The core holds the GIL from its first read of core state to
    its last write and runs no Python code in between (see
    PyHivedCore::schedulePod and ::deleteAllocatedPodByKey in
    core/bindings.cpp), so the lock would serialise nothing there that the GIL
    does not, and the native methods themselves turn a core error into the
    WebServerError that `_call` raises.
    """

    def __init__(self, config: Config):
        self._lock = threading.RLock()
        try:
            self._core = hivedcore.HivedCore(normalize_spec(config))
        except hivedcore.CoreError as e:
            raise WebServerError(getattr(e, "code", 500), str(e)) from e
        self._config = config
        # schedule_pod(spec, pod_key, suggested_nodes=None, phase=FILTERING,
        #              commit=False) -> ScheduleResult
        # One whole filter decision in one core call: validate and default the
        # spec (as validate_pod_scheduling_spec does), decide, and with
        # commit=True add the pod as allocated on a bind decision.
        # suggested_nodes=None stands for every node of the cluster.
        self.schedule_pod = self._core.schedule_validated_pod
        # delete_allocated_pod_by_key(pod_key) -> bool
        # Releases the allocated pod the core holds under pod_key, exactly as
        # delete_allocated_pod(spec, info, pod_key) does for the spec and bind
        # info the pod was added with. False, with nothing changed, if the core
        # holds no such pod (never added, released already, or added before a
        # restart and not replayed yet): fall back to the spec / info form then.
        self.delete_allocated_pod_by_key = self._core.delete_validated_pod_by_key

    def _call(self, fn, *args):
        with self._lock:
            try:
                return fn(*args)
            except hivedcore.CoreError as e:
                raise WebServerError(getattr(e, "code", 400), str(e)) from e

    # --- node events ---
    def add_node(self, name: str, healthy: bool = True) -> None:
        self._call(self._core.set_node_healthy, name, healthy)

    def update_node(self, name: str, healthy: bool) -> None:
        self._call(self._core.set_node_healthy, name, healthy)

    def delete_node(self, name: str) -> None:
        self._call(self._core.set_node_healthy, name, False)

    def set_bad_node(self, name: str) -> None:
        self._call(self._core.set_node_healthy, name, False)

    def set_healthy_node(self, name: str) -> None:
        self._call(self._core.set_node_healthy, name, True)

    def set_leaf_cell_healthy(self, node: str, leaf_index: int, healthy: bool) -> None:
        """GPU/xGMI-level health: marks one leaf cell; badness rolls up to the
        pair/quad/node cells. Independent of node-level health."""
        self._call(self._core.set_leaf_cell_healthy, node, leaf_index, healthy)

    def set_xgmi_link_healthy(self, node: str, a: int, b: int, healthy: bool,
                              gbps: float = 0.0) -> None:
        """First-class xGMI link health: a degraded link between GPUs a and b
        of one node makes multi-GPU placements avoid co-placing the two
        endpoints, while both GPUs stay schedulable for 1-GPU work (unlike
        set_leaf_cell_healthy, which removes a GPU entirely)."""
        self._call(self._core.set_xgmi_link_healthy, node, a, b, healthy, gbps)

    def get_xgmi_links(self, node: str) -> List[dict]:
        """Per-node link table: [{a, b, gbps, healthy}, ...]."""
        return self._call(self._core.xgmi_links, node)

    def all_nodes(self) -> List[str]:
        return self._call(self._core.all_nodes)

    def bad_nodes(self) -> List[str]:
        return self._call(self._core.bad_nodes)

    # --- scheduling ---
    # The core reads PodSchedulingSpec / PodBindInfo objects by attribute, so
    # they cross the boundary as they are (no to_dict() round trip).
    def schedule(
        self,
        spec: PodSchedulingSpec,
        pod_key: str,
        suggested_nodes: List[str],
        phase: str = FILTERING,
    ) -> ScheduleResult:
        """Decide only: the spec is taken as it is (already validated and
        defaulted by the caller), nothing is committed."""
        if suggested_nodes is None:
            raise TypeError("suggested_nodes must be a sequence of node names, not NoneType")
        return self._call(self._core.schedule_pod, spec, pod_key, suggested_nodes, phase,
                          False, False)

    def add_unallocated_pod(self, spec: PodSchedulingSpec, pod_key: str) -> None:
        pass  # parity: reference AddUnallocatedPod is a no-op

    def delete_unallocated_pod(self, spec: PodSchedulingSpec, pod_key: str) -> None:
        self._call(self._core.delete_unallocated_pod, spec, pod_key)

    def add_allocated_pod(self, spec: PodSchedulingSpec, info: PodBindInfo, pod_key: str) -> None:
        self._call(self._core.add_allocated_pod, spec, info, pod_key)

    def delete_allocated_pod(self, spec: PodSchedulingSpec, info: PodBindInfo, pod_key: str) -> None:
        self._call(self._core.delete_allocated_pod, spec, info, pod_key)

    # --- inspect ---
    def get_all_affinity_groups(self) -> List[dict]:
        return self._call(self._core.get_all_affinity_groups)

    def get_affinity_group(self, name: str) -> dict:
        return self._call(self._core.get_affinity_group, name)

    def get_cluster_status(self) -> dict:
        return self._call(self._core.get_cluster_status)

    def get_physical_cluster_status(self) -> list:
        return self._call(self._core.get_physical_cluster_status)

    def get_all_virtual_clusters_status(self) -> dict:
        return self._call(self._core.get_all_virtual_clusters_status)

    def get_virtual_cluster_status(self, vc: str) -> list:
        return self._call(self._core.get_virtual_cluster_status, vc)

    def schedule_count(self) -> int:
        return self._call(self._core.schedule_count)
