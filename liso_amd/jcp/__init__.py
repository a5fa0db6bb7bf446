"""Ground segmentation (reference liso/jcp)."""
