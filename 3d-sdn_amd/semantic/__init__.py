"""The semantic branch's tail on the device: decoder scores to label maps and to the evaluation's integers.  The
segmentation network itself (semantic/models.py) is the caller's."""
