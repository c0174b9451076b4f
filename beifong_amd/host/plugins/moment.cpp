// src/integrators/moment.cpp:27-131 — MomentIntegrator: next to every channel of the nested integrator an "m2_" channel with
// the sum of the squared samples (BF_FLAG_MOMENT; the kernels' kMoment variants).  The reference takes several nested
// integrators; the engine runs one estimator per path, so exactly one is accepted.
#include "../render.h"
using namespace bfh;
class MomentIntegrator final : public SamplingIntegrator {
public:
    explicit MomentIntegrator(const Properties &props) : SamplingIntegrator(props) {
        for (auto &kv : props.objects()) {
            auto *in = dynamic_cast<SamplingIntegrator *>(kv.second.get());
            if (!in) Throw("Child objects must be of type 'SamplingIntegrator'!");                       // :38
            if (m_integrator)
                Throw("moment: more than one nested integrator (\"%s\" after \"%s\"): the reference samples each of them per ray, "
                      "this engine runs one estimator per path — render them one at a time",
                      kv.first.c_str(), m_name.c_str());
            m_integrator = in;
            m_name = kv.first;
        }
        if (!m_integrator) Throw("Must specify a sub-integrator!");
        if (fast_math())
            Throw("moment: \"fast_math\" on the moment integrator or below it is refused: the fast-arithmetic tolerance contract "
                  "says nothing about squared samples (BF_FLAG_MOMENT | BF_FLAG_FAST)");
        check_exact_sum();      // "exact_sum" on the moment integrator or below it: refused by name
        // render until converged (not reference properties; bf_render_converge).  rel_stderr = 0: one render, as ever
        m_converge.rel_stderr = props.float_("rel_stderr", 0.f);
        if (!(m_converge.rel_stderr >= 0.f)) Throw("moment: \"rel_stderr\" must not be negative (0 = off)");
        const bool on = m_converge.rel_stderr > 0.f;
        for (const char *name : {"significance", "max_passes", "passes_per_round"})
            if (!on && props.has_property(name)) Throw("moment: \"%s\" without \"rel_stderr\" > 0 has nothing to act on", name);
        m_converge.significance = props.float_("significance", m_converge.significance);
        if (!(m_converge.significance >= 0.f && m_converge.significance <= 1.f)) Throw("moment: \"significance\" must lie in [0, 1]");
        const int64_t per_round = props.int_("passes_per_round", 0), max_passes = props.int_("max_passes", m_converge.max_passes);
        if (per_round < 0 || per_round > 65535) Throw("moment: \"passes_per_round\" must lie in [0, 65535] (0: 4, or 1 for a multi-pixel film)");
        if (max_passes < 1 || max_passes > (1 << 24)) Throw("moment: \"max_passes\" must lie in [1, 2^24]");
        if (per_round > 0 && max_passes % per_round != 0)
            Throw("moment: \"max_passes\" (%lld) must be a multiple of \"passes_per_round\" (%lld)", (long long) max_passes, (long long) per_round);
        m_converge.passes_per_round = (uint32_t) per_round;
        m_converge.max_passes = (uint32_t) max_passes;
    }
    const ConvergeSpec *converge() const override { return m_converge.rel_stderr > 0.f ? &m_converge : nullptr; }
    std::vector<std::string> aov_names() const override {
        bf_launch lp{};
        m_integrator->configure(lp);
        std::vector<std::string> r;
        if (lp.mode == BF_MODE_RECEIVE_RAW) {
            // receive(): no counterpart in the reference; the ADC cell is Y A W [nested AOVs] m2_Y (include/beifong_hip.h)
            r = m_integrator->aov_names();
            r.push_back("m2_Y");
            return r;
        }
        for (auto &name : m_integrator->aov_names()) r.push_back(m_name + "." + name);                  // :39-41
        r.push_back(m_name + ".X");                                                                     // :44-46
        r.push_back(m_name + ".Y");
        r.push_back(m_name + ".Z");
        const size_t n = r.size();
        for (size_t i = 0; i < n; ++i) r.push_back("m2_" + r[i]);                                       // :50-52
        return r;
    }
    void configure(bf_launch &lp) const override {
        m_integrator->configure(lp);
        lp.flags |= BF_FLAG_MOMENT;
    }
    int max_depth() const override { return m_integrator->max_depth(); }
    bool doppler() const override { return m_integrator->doppler(); }
    bool fast_math() const override { return SamplingIntegrator::fast_math() || m_integrator->fast_math(); }
    bool exact_sum() const override { return SamplingIntegrator::exact_sum() || m_integrator->exact_sum(); }
    int rr_depth() const override { return m_integrator->rr_depth(); }
private:
    ref<SamplingIntegrator> m_integrator;
    std::string m_name;
    ConvergeSpec m_converge;
};
BF_EXPORT_PLUGIN(MomentIntegrator, "SamplingIntegrator", "moment", "Moment integrator")
