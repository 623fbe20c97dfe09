"""Drop-in for how-do-vits-work-transformer/ops/adversarial.py: the perturbations of the noise-robustness experiment ("Convs are
vulnerable to high-frequency noise, MSAs to low-frequency noise") with the reference's names and signatures.

  * `Random(model=None, *, eps=0.007, gpu=True)` - sign noise: xs + eps * sign(randn), the draw taken on the CPU from the global generator
    as the reference takes it (adversarial.py:99-121).
  * `FreqAttack(attack, *, f, s=0.2)` - the perturbation of `attack` restricted to the frequency band of centre f and half-width s
    (adversarial.py:124-175), through dehaze_hip.freq_noise.band_noise: the float64 HIP kernel on fp32 device tensors, the reference's
    ATen formula elsewhere or with DHZ_FREQ_NOISE=0.

FGSM and PGD are NOT here: they differentiate a classification loss (softmax over the model's output, CrossEntropyLoss), which a dehazing
model does not have.  The kernel's `delta` is general, so a gradient-sign attack on a restoration loss can be wrapped in FreqAttack the
same way once it exists.
"""
import torch

from dehaze_hip import freq_noise


class Random:

    def __init__(self, model=None, *, eps=0.007, gpu=True):
        super().__init__()
        self.eps = eps
        self.gpu = gpu

    def draw(self, xs):
        """the reference's draw for a batch shaped like xs: CPU, global generator, moved to xs.device"""
        b, c, h, w = xs.shape
        return torch.randn([b, c, h, w]).to(xs.device)

    def __call__(self, xs, ys):
        xs = xs.clone().detach()
        ys = ys.clone().detach()
        if self.gpu:
            xs = xs.cuda()
            ys = ys.cuda()
        xs_adv = xs + self.eps * self.draw(xs).sign()
        return xs_adv.detach(), ys


class FreqAttack:

    def __init__(self, attack, *, f, s=0.2):
        super().__init__()
        self.attack = attack
        self.f = f
        self.s = s

    def __call__(self, xs, ys):
        w1, w2 = freq_noise.band_widths(self.f, self.s, xs.shape[-1])
        if isinstance(self.attack, Random):
            # the reference forms xs + eps * sign(draw) - xs in fp32; the band filter takes eps and the draw's sign as they are
            xs = xs.clone().detach()
            ys = ys.clone().detach()
            if self.attack.gpu:
                xs = xs.cuda()
                ys = ys.cuda()
            draw = self.attack.draw(xs).to(xs.dtype)
            return freq_noise.band_noise(xs, draw, w1, w2, scale=self.attack.eps, take_sign=True), ys
        xs_adv, ys = self.attack(xs, ys)
        xs = xs.to(xs_adv.device)
        return freq_noise.band_noise(xs, xs_adv - xs, w1, w2), ys
