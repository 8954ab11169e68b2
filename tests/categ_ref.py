"""Stock torch.nn restatement of class-conditional MoCoGAN on the Neural-ODE generators: models/mocogan.py (categorical
latent :231-247,259-269, CategoricalVideoDiscriminator :167-182) and models/mocogan_ode.py (the ODE motion latent), on top
of oracle.ode_ref.  oracle.mocogan_ref asserts dim_z_category == 0, so the categorical variants live here.  CPU, fp32 (or
fp64 after .double()); the latent draws consume NumPy's and torch's CPU generators in the reference's order: content
(np.random.normal), classes (ONE np.random.randint(C, size=n)), motion noise (torch.randn).

The training objective is MoCoGAN's InfoGAN form; the reference repository ships no script that trains with categories, so
train_step below restates the objective GanTrainer documents (parity with a reference script is unpinned)."""
import numpy as np
import torch
import torch.nn as nn

from oracle import mocogan_ref as M
from oracle import ode_ref


class Generator(nn.Module):
    def __init__(self, n_channels, dim_z_content, dim_z_category, dim_z_motion, video_length, dim_hidden=None, ngf=64,
                 mnist=True, ode_method="rk4"):
        super().__init__()
        self.n_channels, self.dim_z_content, self.dim_z_category = n_channels, dim_z_content, dim_z_category
        self.dim_z_motion, self.video_length = dim_z_motion, video_length
        self.recurrent = nn.GRUCell(dim_z_motion, dim_z_motion)
        self.main = M._decoder(dim_z_motion + dim_z_category + dim_z_content, ngf, n_channels, mnist)
        self.ode_fn = M.OdeRhs(dim_z_motion, dim_hidden if dim_hidden else dim_z_motion)
        self.linear = M._prenet(dim_z_motion)
        self.ode_method = ode_method

    def _dtype(self):
        return self.ode_fn.fn[0].weight.dtype

    def sample_z_content(self, n, video_len=None):
        T = video_len or self.video_length
        c = np.random.normal(0, 1, (n, self.dim_z_content)).astype(np.float32)
        return torch.from_numpy(np.repeat(c, T, axis=0)).to(self._dtype())

    def sample_z_categ(self, n, video_len=None):
        T = video_len or self.video_length
        if self.dim_z_category <= 0:
            return None, np.zeros(n)
        classes = np.random.randint(self.dim_z_category, size=n)
        one_hot = np.zeros((n, self.dim_z_category), dtype=np.float32)
        one_hot[np.arange(n), classes] = 1
        return torch.from_numpy(np.repeat(one_hot, T, axis=0)).to(self._dtype()), classes

    def sample_z_m(self, n, video_len=None):
        T = video_len or self.video_length
        x = self.linear(torch.randn(n, self.dim_z_motion).to(self._dtype()))
        sol = ode_ref.odeint_adjoint(self.ode_fn, x, torch.linspace(0, 1, T).float().to(self._dtype()),
                                     method=self.ode_method)
        return sol.transpose(0, 1).reshape(-1, self.dim_z_motion)

    def sample_z_video(self, n, video_len=None):
        zc = self.sample_z_content(n, video_len)
        zk, classes = self.sample_z_categ(n, video_len)
        zm = self.sample_z_m(n, video_len)
        parts = [zc, zm] if zk is None else [zc, zk, zm]
        return torch.cat(parts, dim=1), classes

    def sample_videos(self, n, video_len=None):
        T = video_len or self.video_length
        z, classes = self.sample_z_video(n, T)
        h = self.main(z.view(z.size(0), z.size(1), 1, 1))
        h = h.view(h.size(0) // T, T, self.n_channels, h.size(3), h.size(3)).permute(0, 2, 1, 3, 4)
        return h, torch.from_numpy(classes)

    def sample_images(self, n):
        z, _ = self.sample_z_video(n * self.video_length * 2)
        j = np.sort(np.random.choice(z.size(0), n, replace=False)).astype(np.int64)
        z = z[j]
        return self.main(z.view(z.size(0), z.size(1), 1, 1)), None


class CategoricalVideoDisc(M.VideoDisc):
    def __init__(self, n_channels, dim_categorical, n_output_neurons=1, ndf=64, ksize=4):
        super().__init__(n_channels, n_output_neurons=n_output_neurons + dim_categorical, ndf=ndf, ksize=ksize)
        self.dim_categorical = dim_categorical

    def split(self, x):
        return x[:, :x.size(1) - self.dim_categorical], x[:, x.size(1) - self.dim_categorical:]

    def forward(self, x):
        h = self.main(x)                              # [B, n_out + C, Do, Ho, Wo]
        if h.shape[2:].numel() == 1:
            h = h.reshape(x.shape[0], -1)
        return self.split(h)


def cross_entropy(categ, labels):
    """nn.CrossEntropyLoss() of a head's class logits against one label per video: [B, C] directly; a patch head
    [B, C, Do, Ho, Wo] with the video's label at every output position (the mean then runs over all positions)."""
    if categ.dim() > 2:
        labels = labels.view(-1, *([1] * (categ.dim() - 2))).expand(categ.shape[0], *categ.shape[2:])
    return nn.functional.cross_entropy(categ, labels)


def build_mnist(C, ngf=64, ndf=64, ode_method="rk4"):
    return (Generator(1, 50, C, 16, 16, ngf=ngf, mnist=True, ode_method=ode_method),
            CategoricalVideoDisc(1, C, ksize=2, ndf=ndf), M.PatchImageDisc(1, ndf=ndf))


def train_step(gen, dis_vid, dis_img, opts, real_imgs, real_vids, real_labels, d_iters=2, log=None):
    """One outer iteration of the categorical objective.  -> (dis_img_loss, dis_vid_loss, gen_loss) of the last inner pass.
    log (a list): every optimiser step's loss in order."""
    gen_opt, vid_opt, img_opt = opts
    bce, ce = nn.BCEWithLogitsLoss(), cross_entropy
    B = real_imgs[0].shape[0]
    for i in range(d_iters):
        li = M.d_image_step(gen, dis_img, img_opt, real_imgs[i], bce, B)
        vid_opt.zero_grad()
        pr, cr = dis_vid(real_vids[i].transpose(1, 2))
        with torch.no_grad():
            fake, _ = gen.sample_videos(B)
        pf, _ = dis_vid(fake)
        lv = bce(pr, torch.ones_like(pr)) + bce(pf, torch.zeros_like(pf)) + ce(cr, real_labels[i])
        lv.backward()
        vid_opt.step()
        if log is not None:
            log += [li.detach(), lv.detach()]
    gen_opt.zero_grad()
    fake_vid, classes = gen.sample_videos(B)
    fake_img, _ = gen.sample_images(B)
    pv, cv = dis_vid(fake_vid)
    pi, _ = dis_img(fake_img)
    lg = bce(pv, torch.ones_like(pv)) + bce(pi, torch.ones_like(pi)) + ce(cv, classes)
    lg.backward()
    gen_opt.step()
    if log is not None:
        log.append(lg.detach())
    return li.detach(), lv.detach(), lg.detach()
