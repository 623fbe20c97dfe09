"""Drop-in for FFA_model/models/PerceptualLoss.py: LossNetwork, exported as PerLoss by FFA_model/models/__init__.py - the perceptual
term of FFA-Net's own recipe (FFA_main.py --perloss).  The implementation is dehaze_hip/perceptual.py: on a HIP device the VGG16[:16]
features run on the Winograd engine and the squared-error taps on dhz_mse_pair_fwd / _bwd."""
from dehaze_hip.perceptual import LossNetwork, seeded_vgg16_init_, vgg16_feature_layers  # noqa: F401

PerLoss = LossNetwork
