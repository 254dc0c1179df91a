from .smokephys_net import SmokePhysNet, SmokePhysNet3D, ChaosTransformerLayer
from .chaos_attention import ChaosAttention
from .physics_regularizer import PhysicsRegularizer
from .encoder import HipEncoder
from .encoder3d import Encoder3D, HipEncoder3D, hip_volume_input_grad_supported
from .graphed import GraphedSmokePhysNet

__all__ = ["SmokePhysNet", "SmokePhysNet3D", "ChaosTransformerLayer", "ChaosAttention", "PhysicsRegularizer", "HipEncoder", "HipEncoder3D", "Encoder3D", "GraphedSmokePhysNet",
           "hip_volume_input_grad_supported"]
