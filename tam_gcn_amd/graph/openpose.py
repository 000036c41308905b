"""OpenPose 18-keypoint skeleton graph, the layout ST-GCN was published on:
0 nose, 1 neck, 2-4 right shoulder / elbow / wrist, 5-7 left arm, 8-10 right hip / knee / ankle, 11-13 left leg,
14 / 15 right / left eye, 16 / 17 right / left ear.

Stored as a parent table (joint k+1 -> parent, 0 = root) like graph/ucla.py; the neck is the root.  Its inward links
(child, parent) are (4,3) (3,2) (7,6) (6,5) (13,12) (12,11) (10,9) (9,8) (11,5) (8,2) (5,1) (2,1) (0,1) (15,0) (14,0)
(17,15) (16,14).
"""
from . import tools

#           1  2  3  4  5  6  7  8  9 10  11 12  13  14 15 16  17  18
_PARENTS = (2, 0, 2, 3, 4, 2, 6, 7, 3, 9, 10, 6, 12, 13, 1, 1, 15, 16)

num_node = len(_PARENTS)
self_link, inward, outward, neighbor = tools.links_from_parents(_PARENTS)


class Graph(tools.SpatialGraph):
    parents = _PARENTS

    def __init__(self, labeling_mode='spatial', scale=1):
        super().__init__(labeling_mode)
