"""The label function of the reference's liso/datasets/argoverse2/create.py (:357-383) under its module path
(liso_amd/datasets/flow_labels.py)."""
from liso_amd.datasets.flow_labels import update_dynamic_flow  # noqa: F401
