"""MI355X-native cost-volume hot path of Practical Deep Stereo (NeurIPS 2018).

Matching -> Regularization -> SubpixelMap behind the reference's module surfaces, computed by
hand-written HIP kernels for gfx950 (libpds_hip.so, C ABI in include/pds_hip.h).
"""
from practicaldeepstereo_nips2018_amd import errors
from practicaldeepstereo_nips2018_amd.consistency import left_right_check
from practicaldeepstereo_nips2018_amd.embedding import Embedding
from practicaldeepstereo_nips2018_amd.estimator import SubpixelMap
from practicaldeepstereo_nips2018_amd.loss import SubpixelCrossEntropy
from practicaldeepstereo_nips2018_amd.matching import Matching, MatchingOperation
from practicaldeepstereo_nips2018_amd.median import MedianFiltered, median_filter
from practicaldeepstereo_nips2018_amd.mesh import TriangleMesh, TriangleMeshEntry, triangle_mesh
from practicaldeepstereo_nips2018_amd.network import PdsNetwork
from practicaldeepstereo_nips2018_amd.normals import SurfaceNormals, surface_normals
from practicaldeepstereo_nips2018_amd.pyramid import disparity_pyramid, intensity_pyramid, pyramid_camera, pyramid_matrix
from practicaldeepstereo_nips2018_amd.point_cloud import PointCloud, PointCloudEntry, point_cloud, save_ply
from practicaldeepstereo_nips2018_amd.rectification import StereoRig, remap, reproject, stereo_rectify
from practicaldeepstereo_nips2018_amd.registration import RegisteredDepth, register_depth
from practicaldeepstereo_nips2018_amd.regularization import (ContractionBlock3d, ExpansionBlock3d,
                                                            Regularization)
from practicaldeepstereo_nips2018_amd.speckle import SpeckleFiltered, region_sizes, speckle_filter
from practicaldeepstereo_nips2018_amd.tsdf import SurfaceMesh, SurfacePoints, TsdfVolume
from practicaldeepstereo_nips2018_amd.tracking import (ColorTracking, IcpColorSystem, IcpSolution, IcpSystem, Tracking,
                                                       icp_color_system, icp_solve, icp_system, icp_system_robust, se3_exp)
from practicaldeepstereo_nips2018_amd.tsdf_color import ColorRaycast, ColorTsdfVolume
from practicaldeepstereo_nips2018_amd.tsdf_raycast import Raycast, depth_to_disparity

__all__ = ['errors', 'Embedding', 'SubpixelMap', 'SubpixelCrossEntropy', 'Matching', 'MatchingOperation', 'PdsNetwork', 'ContractionBlock3d',
           'ExpansionBlock3d', 'Regularization', 'left_right_check', 'StereoRig',
           'stereo_rectify', 'remap', 'reproject', 'speckle_filter', 'region_sizes', 'SpeckleFiltered',
           'median_filter', 'MedianFiltered', 'point_cloud', 'PointCloud', 'PointCloudEntry',
           'register_depth', 'RegisteredDepth', 'surface_normals', 'SurfaceNormals', 'save_ply',
           'triangle_mesh', 'TriangleMesh', 'TriangleMeshEntry', 'TsdfVolume', 'SurfacePoints', 'SurfaceMesh',
           'Raycast', 'ColorTsdfVolume', 'ColorRaycast',
           'depth_to_disparity', 'icp_system', 'icp_solve', 'se3_exp', 'IcpSystem', 'IcpSolution', 'Tracking',
           'disparity_pyramid', 'pyramid_matrix', 'pyramid_camera', 'icp_system_robust',
           'intensity_pyramid', 'icp_color_system', 'IcpColorSystem', 'ColorTracking']
