"""COCO 17-keypoint skeleton graph (the layout of COCO-pose / YOLO-pose estimators):
0 nose, 1 / 2 left / right eye, 3 / 4 ears, 5 / 6 shoulders, 7 / 8 elbows, 9 / 10 wrists, 11 / 12 hips, 13 / 14 knees,
15 / 16 ankles.

The topology is stored as a parent table (joint k+1 -> parent, 0 = root) like graph/ucla.py; the nose is the root, the
shoulders hang off it, the hips off the shoulders.  17 joints is none of the joint counts CTRGC has dedicated kernels for:
such a graph runs on the run-time-V kernel family.
"""
from . import tools

#           1  2  3  4  5  6  7  8  9 10 11 12 13  14  15  16  17
_PARENTS = (0, 1, 1, 2, 3, 1, 1, 6, 7, 8, 9, 6, 7, 12, 13, 14, 15)

num_node = len(_PARENTS)
self_link, inward, outward, neighbor = tools.links_from_parents(_PARENTS)


class Graph(tools.SpatialGraph):
    parents = _PARENTS

    def __init__(self, labeling_mode='spatial', scale=1):
        super().__init__(labeling_mode)
