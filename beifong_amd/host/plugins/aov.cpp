// src/integrators/aov.cpp:83-150,170-251 — AOVIntegrator (stock Mitsuba): behind X Y Z A W every pixel carries the arbitrary output
// variables named by "aovs" (depth, position, uv, normals, position partials of the first intersection), then the nested
// integrator's own AOVs and its R G B A (BF_FLAG_AOV; the kernels' kAov variants).  The reference takes several nested
// integrators; the engine runs one estimator per path, so exactly one is accepted.
#include "../render.h"
using namespace bfh;
namespace {
std::vector<std::string> tokenize(const std::string &s, const std::string &delim) {      // string::tokenize (string.cpp): empty tokens dropped
    std::vector<std::string> out;
    size_t at = 0;
    while (at <= s.size()) {
        const size_t end = std::min(s.find_first_of(delim, at), s.size());
        if (end > at) out.push_back(s.substr(at, end - at));
        at = end + 1;
    }
    return out;
}
}  // namespace
class AOVIntegrator final : public SamplingIntegrator {
public:
    explicit AOVIntegrator(const Properties &props) : SamplingIntegrator(props) {
        for (const std::string &token : tokenize(props.string("aovs"), ", ")) {                          // :84-135
            const std::vector<std::string> item = tokenize(token, ":");
            // (the reference only warns here and then reads item[1]; there is nothing to go on with)
            if (item.size() != 2 || item[0].empty() || item[1].empty()) Throw("Invalid AOV specification: require <name>:<type> pair");
            static const struct { const char *name; uint32_t type; const char *suffix; } kTypes[] = {
                {"depth", BF_AOV_DEPTH, ""}, {"position", BF_AOV_POSITION, "XYZ"}, {"uv", BF_AOV_UV, "UV"},
                {"geo_normal", BF_AOV_GEO_NORMAL, "XYZ"}, {"sh_normal", BF_AOV_SH_NORMAL, "XYZ"}, {"dp_du", BF_AOV_DP_DU, "XYZ"},
                {"dp_dv", BF_AOV_DP_DV, "XYZ"}, {"duv_dx", BF_AOV_DUV_DX, "UV"}, {"duv_dy", BF_AOV_DUV_DY, "UV"}};
            bool found = false;
            for (const auto &t : kTypes) {
                if (item[1] != t.name) continue;
                found = true;
                m_types.push_back(t.type);
                if (!*t.suffix) m_names.push_back(item[0]);
                for (const char *c = t.suffix; *c; ++c) m_names.push_back(item[0] + "." + *c);
            }
            if (!found) Throw("Invalid AOV type \"%s\"!", item[1].c_str());
        }
        if (m_types.empty()) Throw("aov: \"aovs\" names no AOV: the engine's table needs at least one (BF_FLAG_AOV)");
        if (m_types.size() > BF_MAX_AOVS) Throw("aov: \"aovs\" names %zu AOVs, at most %d", m_types.size(), (int) BF_MAX_AOVS);
        for (auto &kv : props.objects()) {
            auto *in = dynamic_cast<SamplingIntegrator *>(kv.second.get());
            if (!in) Throw("Child objects must be of type 'SamplingIntegrator'!");                       // :140
            if (m_integrator)
                Throw("aov: more than one nested integrator (\"%s\" after \"%s\"): the reference samples each of them per ray, "
                      "this engine runs one estimator per path — render them one at a time",
                      kv.first.c_str(), m_name.c_str());
            m_integrator = in;
            m_name = kv.first;
        }
        if (!m_integrator)
            Throw("aov: no nested integrator: the reference samples each nested integrator per ray, this engine runs one estimator "
                  "per path — name exactly one");
        if (fast_math())
            Throw("aov: \"fast_math\" on the aov integrator or below it is refused: the AOV kernels exist of the exact build only "
                  "(BF_FLAG_AOV | BF_FLAG_FAST)");
        bf_launch lp{};
        m_integrator->configure(lp);
        if (lp.flags & BF_FLAG_MOMENT) Throw("aov: a nested \"moment\" integrator is refused: the AOV kernels carry no second moments (BF_FLAG_AOV | BF_FLAG_MOMENT)");
        if (lp.flags & BF_FLAG_AOV) Throw("aov: a nested \"aov\" integrator is refused: one table per render");
        check_exact_sum();      // "exact_sum" on the aov integrator or below it: refused by name
    }
    std::vector<std::string> aov_names() const override {
        std::vector<std::string> r = m_names;
        for (auto &name : m_integrator->aov_names()) r.push_back(m_name + "." + name);                  // :142-144
        for (const char *c : {".R", ".G", ".B", ".A"}) r.push_back(m_name + c);                         // :146-149
        return r;
    }
    std::vector<uint32_t> aov_types() const override { return m_types; }
    void configure(bf_launch &lp) const override {
        m_integrator->configure(lp);
        lp.flags |= BF_FLAG_AOV;
    }
    bool receive(Scene *, Receiver *) override {
        Throw("aov: receive() is refused: the aov integrator wraps a sampling integrator and writes a film; the ADC has no AOV channels");
    }
    int max_depth() const override { return m_integrator->max_depth(); }
    bool doppler() const override { return m_integrator->doppler(); }
    bool fast_math() const override { return SamplingIntegrator::fast_math() || m_integrator->fast_math(); }
    bool exact_sum() const override { return SamplingIntegrator::exact_sum() || m_integrator->exact_sum(); }
    int rr_depth() const override { return m_integrator->rr_depth(); }
private:
    ref<SamplingIntegrator> m_integrator;
    std::string m_name;
    std::vector<uint32_t> m_types;
    std::vector<std::string> m_names;
};
BF_EXPORT_PLUGIN(AOVIntegrator, "SamplingIntegrator", "aov", "AOV integrator")
